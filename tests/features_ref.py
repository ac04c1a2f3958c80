"""CPU reference of gs_render_features' feature image.

Every channel F_k is composited exactly as a colour channel whose per-splat
value is features[i][k].  The oracle composites whatever floats a record carries
in `r`, `g` and `b` with C = fmaf(c, w, C) and no clamp, all three alike
(ora_composite_records), so three channels at a time are the colour channels of
the frame's own records with r, g, b replaced by three feature columns (zero
pads the last group): the same fragments, order, weights and break rule as the
colour frame, whose alpha must therefore come out unchanged, bit for bit.
Splats that reach no tile get 0, so their rows (NaN included) stay out of the
reference, as they stay out of every list.

features_ref asserts on every call that each such composite's alpha is the
colour frame's and that the plain record composite is the oracle's frame; once
per projection and rule, that one column placed in r, g and b gives three
bit-identical images (which licenses the three-at-a-time use)."""
import numpy as np

from depth_ref import project_zf  # noqa: F401  (the shared projection: records, depth keys, tiles, zF)


def _bits(a, b):
    return int(np.count_nonzero(np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)))


_alike = {}  # (id of the projection's records, rule) -> the projection (kept alive, so the id stays its own)


def _channels_alike(proj, W, H, mode, column):
    from oracle import oracle_py as O
    rec, dkey, _, _ = proj
    key = (id(rec), mode)
    if key in _alike:
        return
    same = rec.copy()
    for ch in "rgb":
        same[ch] = column
    img = O.composite_records(same, dkey, W, H, mode=mode)
    assert _bits(img[..., 0], img[..., 1]) == 0 and _bits(img[..., 0], img[..., 2]) == 0
    _alike[key] = proj


def features_from_projection(scene, V, P, W, H, mode, sh_degree, proj, features):
    """features_ref from a projection computed once (project_zf) and shared between rules and matrices."""
    from oracle import oracle_py as O
    rec, dkey, ntiles, _ = proj
    features = np.asarray(features)
    assert features.ndim == 2 and features.dtype == np.float32 and features.shape[0] == rec.shape[0]
    K = features.shape[1]
    colour, _ = O.render(scene, V, P, W, H, sh_degree=sh_degree, mode=mode)
    again = O.composite_records(rec, dkey, W, H, mode=mode)
    assert _bits(again, colour) == 0  # the record composite is the oracle's frame
    vis = ntiles > 0
    zero = np.zeros(rec.shape[0], np.float32)
    cols = [np.where(vis, features[:, k], np.float32(0.0)).astype(np.float32) for k in range(K)]
    _channels_alike(proj, W, H, mode, cols[0])
    out = np.empty((H, W, K), np.float32)
    for g in range(0, K, 3):
        frec = rec.copy()
        for j, ch in enumerate("rgb"):
            frec[ch] = cols[g + j] if g + j < K else zero
        img = O.composite_records(frec, dkey, W, H, mode=mode)
        assert _bits(img[..., 3], colour[..., 3]) == 0  # alpha untouched: same fragments, weights and breaks
        n = min(3, K - g)
        out[..., g:g + n] = img[..., :n]
    out.setflags(write=False)
    colour.setflags(write=False)
    return out, colour


def features_ref(scene, V, P, W, H, mode, features, sh_degree=0, with_colour=False):
    """The feature image (H, W, K) float32 of the frame; with_colour: also the oracle's colour frame."""
    feats, colour = features_from_projection(scene, V, P, W, H, mode, sh_degree,
                                             project_zf(scene, V, P, W, H, sh_degree), features)
    return (feats, colour) if with_colour else feats
