"""What the CPU oracle makes of degenerate and non-finite splat values
(degenerate_zoo.py): the contract for values outside the well-formed range
(DESIGN.md §2.10), written down as measured on the oracle alone.  No GPU:
these pins are what makes the GPU comparison of test_gpu_degenerate.py
non-vacuous (the classes reach the records and the frames, the ordinary
pipeline around them is still judged), and every number here is the
oracle's own output, never the HIP path's.

Measured frame shares (tile rule; live50 is equal, mlab within 0.2 %):
  333 x 211    NaN pixels 1.13 %, alpha > 0 on 99.3 %, 26 pixels with alpha > 1
  1037 x 531   NaN pixels 0.99 %, alpha > 0 on 99.4 %, 299 pixels with alpha > 1
  dense        NaN 4.1 % / 3.8 %, alpha >= 0.99 on 97.7 % / 97.1 %
No value is infinite, and no pixel of these frames ends with alpha < 0: the
opacity -0.5 fragments are composited (alpha plays no part in the coverage
test), over the full-frame classes' tint."""
import functools

import numpy as np
import pytest

from degenerate_zoo import K, SH_CLASSES, same_frame, same_records, thresholds, zoo
from oracle import oracle_py as O

SHAPES = [(333, 211), (1037, 531)]

# class -> (visible of K at 333 x 211, at 1037 x 531; full-frame rects among them at either shape;
#           the other visible rects: "small" = every one within 16 x 16 px, "ordinary" = median area
#           under 100 px, None = there are none; NaN record fields, () = every visible record finite)
PINS = {
    "rot_zero":            (0, 0, 0, 0, None, ()),          # qs = 0: 1/sqrt(0) = inf, 0 * inf = NaN radii: culled
    "rot_1e-20":           (K, K, 0, 0, "ordinary", ()),    # qs subnormal, still normalised
    "rot_1e19":            (K, K, 0, 0, "ordinary", ()),    # qs = inf: q * (1/inf) = 0, R = identity
    "rot_nan":             (0, 0, 0, 0, None, ()),
    "scale_zero":          (K, K, 0, 0, "small", ()),       # the + 1e-4 floor on the 2D covariance
    "scale_axis_zero":     (K, K, 0, 0, "ordinary", ()),
    "scale_inf":           (0, 0, 0, 0, None, ()),          # inf * 0 = NaN in M = R S
    "scale_1e19":          (K, K, K, K, None, ()),          # covariance overflows: full-frame rect, zero conic
    "scale_1e10":          (1, 0, 1, 0, None, ()),          # axes normalise to (0, 0): culled, but for 1 (b = 1.2e18, b^2 finite) at 333 x 211
    "scale_1e-30":         (K, K, 0, 0, "small", ()),
    "scale_negated":       (K, K, 0, 0, "ordinary", ()),    # Sigma = M M^T: the sign cancels
    "scale_nan":           (0, 0, 0, 0, None, ()),
    "scale_needle":        (8, 10, 8, 9, "any", ()),        # split: 40 / 38 culled; one half-frame rect at 1037 x 531
    "opacity_zero":        (K, K, 0, 0, "ordinary", ()),
    "opacity_one":         (K, K, 0, 0, "ordinary", ()),
    "opacity_1.5":         (K, K, 0, 0, "ordinary", ()),
    "opacity_-0.5":        (K, K, 0, 0, "ordinary", ()),
    "opacity_nan":         (K, K, 0, 0, "ordinary", ("opacity",)),
    "color_nan":           (K, K, 0, 0, "ordinary", ("rgb",)),  # sh 0 only: the SH path's clamp swallows the NaN
    "color_range":         (K, K, 0, 0, "ordinary", ()),
    "pos_x_nan":           (0, 0, 0, 0, None, ()),
    "pos_y_inf":           (0, 0, 0, 0, None, ()),
    "pos_z_-1e30":         (0, 0, 0, 0, None, ()),
    "sh_nan":              (K, K, 0, 0, "ordinary", ()),    # fminf(fmaxf(NaN, 0), 1) = 0
    "sh_inf":              (K, K, 0, 0, "ordinary", ()),
    "sh_1e30":             (K, K, 0, 0, "ordinary", ()),
    "sh_dc_zero_nan_rest": (K, K, 0, 0, "ordinary", ()),    # all-zero f_dc: colour 0 whatever the rest holds
    "rot_zero_runs":       (0, 0, 0, 0, None, ()),
}


@functools.lru_cache(maxsize=None)
def _frame(W, H, mode, dense=False, cap=0):
    sc, V, P, _ = zoo(W, H, 0, dense)
    ref, st = O.render(sc, V, P, W, H, mode=mode, cap=cap)
    ref.setflags(write=False)
    return ref, st


@pytest.mark.parametrize("sh", [0, 3])
@pytest.mark.parametrize("W,H", SHAPES)
def test_classes(built, W, H, sh):
    sc, V, P, classes = zoo(W, H, sh)
    rec, dk, nt = O.project(sc, V, P, W, H, sh_degree=sh)
    assert set(classes) == {n for n in PINS if sh > 0 or n not in SH_CLASSES} | {"untouched"}
    assert sum(len(i) for i in classes.values()) == sc.n == 6000
    for name, idx in classes.items():
        vis = nt[idx] > 0
        if name == "untouched":  # the ordinary pipeline is still judged: every untouched base splat is visible
            assert len(idx) == (4576 if sh == 0 else 4384) and vis.all()
            assert np.isfinite(rec[idx].view(np.uint32).reshape(-1, 12)[:, :10].view(np.float32)).all()
            continue
        v333, v1037, f333, f1037, rest, nanf = PINS[name]
        want_vis, want_full = (v333, f333) if W == 333 else (v1037, f1037)
        assert len(idx) == (320 if name == "rot_zero_runs" else K)
        assert int(vis.sum()) == want_vis, (name, int(vis.sum()))
        assert np.all(dk[idx][~vis] == 0)
        r = rec[idx][vis]
        w = (r["rect_hi"] & 0xFFFF) - (r["rect_lo"] & 0xFFFF) + 1
        h = (r["rect_hi"] >> 16) - (r["rect_lo"] >> 16) + 1
        full = (w == W) & (h == H)
        assert int(full.sum()) == want_full, (name, int(full.sum()))
        other = ~full
        if rest is None:
            assert not other.any(), name
        elif rest == "small":
            assert other.any() and (w[other] <= 16).all() and (h[other] <= 16).all(), name
        elif rest == "ordinary":
            assert other.any() and np.median((w * h)[other]) < 100, (name, np.median((w * h)[other]))
        f = r.view(np.uint32).reshape(-1, 12)[:, :10].view(np.float32)
        assert not np.isinf(f).any(), name
        nan = np.isnan(f)
        if nanf == ("opacity",):
            assert nan[:, 6].all() and not np.delete(nan, 6, axis=1).any()
        elif nanf == ("rgb",) and sh == 0:  # one channel each, the others as given
            assert (nan[:, 7:10].sum(axis=1) == 1).all() and not nan[:, :7].any()
        else:
            assert not nan.any(), name
    if sh > 0:  # the all-zero f_dc quirk wins over a NaN rest
        q = rec[classes["sh_dc_zero_nan_rest"]]
        assert (q["r"] == 0).all() and (q["g"] == 0).all() and (q["b"] == 0).all()


@pytest.mark.parametrize("mode", ["tile", "live50", "mlab"])
@pytest.mark.parametrize("W,H", SHAPES)
def test_frame_conditions(built, W, H, mode):
    ref, st = _frame(W, H, mode)
    nan = np.isnan(ref).any(axis=-1)
    a = ref[..., 3]
    print(f"{W}x{H} {mode}: NaN pixels {nan.mean():.4f}, alpha > 0 {np.mean(a > 0):.4f}, alpha < 0 {int((a < 0).sum())}, "
          f"alpha > 1 {int((a > 1).sum())}, pairs {st['pairs']}")
    assert 0 < nan.mean() <= 0.05
    assert not np.isinf(ref).any()
    assert ((a < 0) | (a > 1)).any()
    assert np.mean(a > 0) >= 0.95
    assert same_frame(ref, ref) == (0, 0)
    other = ref.copy()
    isn = np.isnan(other)
    other[isn] = -other[isn]          # a NaN's sign is not compared ...
    assert (other.view(np.uint32) != ref.view(np.uint32)).any()
    assert same_frame(other, ref) == (0, 0)
    y, x = np.argwhere(~nan)[0]
    other[y, x, 3] = np.nextafter(other[y, x, 3], np.float32(2))  # ... a bit of a number is,
    assert same_frame(other, ref) == (0, 1)
    y, x = np.argwhere(nan)[0]
    other[y, x] = 0.0                 # and so is a NaN's place
    assert same_frame(other, ref)[0] == 1


@pytest.mark.parametrize("mode", ["tile", "live50", "mlab"])
def test_negative_alpha_is_composited(built, mode):
    """The discards are on depth and on the gaussian (tile.metal:187-195); the
    alpha = opacity * g of :197 is composited whatever its sign.  The opacity
    -0.5 class alone: every covered pixel ends with alpha < 0 under the tile
    and live-50 rules (T grows past 1)."""
    W, H = 333, 211
    sc, V, P, classes = zoo(W, H)
    ref, st = O.render(sc.subset(classes["opacity_-0.5"]), V, P, W, H, mode=mode)
    a = ref[..., 3]
    assert st["visible"] == K and not np.isnan(ref).any()
    if mode == "mlab":
        assert (ref != 0).any()
    else:
        assert (a < 0).sum() > 4 * K and not (a > 0).any()


@pytest.mark.parametrize("mode,cap", [("tile", 32), ("live50", 50)])
@pytest.mark.parametrize("W,H", SHAPES)
def test_dense_frame_conditions(built, W, H, mode, cap):
    """The dense variant (the depth-cut and cap tests): at least a quarter of
    the frame saturated, at most a tenth NaN, and the cap binds."""
    ref, _ = _frame(W, H, mode, dense=True)
    nan = np.isnan(ref).any(axis=-1)
    a = ref[..., 3]
    print(f"{W}x{H} {mode} dense: NaN pixels {nan.mean():.4f}, alpha >= 0.99 {np.mean(a >= 0.99):.4f}")
    assert np.mean(a >= 0.99) >= 0.25
    assert 0 < nan.mean() <= 0.10
    assert not np.isinf(ref).any()
    assert ((a < 0) | (a > 1)).any()
    sc, V, P, classes = zoo(W, H, 0, True)
    _, _, nt = O.project(sc, V, P, W, H)
    assert (nt[classes["untouched"]] > 0).all()
    capped, _ = _frame(W, H, mode, dense=True, cap=cap)
    assert same_frame(capped, ref) != (0, 0)


@pytest.mark.parametrize("sh", [0, 3])
@pytest.mark.parametrize("W,H", SHAPES)
def test_thresholds(built, W, H, sh):
    """zFront 0.0009 is culled (the fragment discard below 0.001), 0.001 and
    0.0011 are not; the depth key 0x7C00 - f16bits(zFront) reaches 0 where
    the half overflows (65520 rounds to infinity, 65519 to 65504)."""
    sc, V, P, d = thresholds(W, H)
    rec, dk, nt = O.project(sc, V, P, W, H, sh_degree=sh)
    assert d.tolist() == np.float32([0.0009, 0.001, 0.0011, 65503, 65504, 65519, 65520, 1e5]).tolist()
    assert nt[0] == 0 and (nt[1:] > 0).all(), nt
    want = [0x7C00 - O.f16_bits(float(z)) for z in d]
    assert dk[1:].tolist() == want[1:]
    assert [O.f16_bits(float(z)) for z in d[3:]] == [0x7BFF, 0x7BFF, 0x7BFF, 0x7C00, 0x7C00]
    assert dk[5] == 1 and dk[6] == 0 and dk[7] == 0 and dk[1] > dk[2] > 1
    assert np.isfinite(rec[1:].view(np.uint32).reshape(-1, 12)[:, :10].view(np.float32)).all()


def test_ply_route(built, tmp_path):
    """Raw PLY values whose activations leave the well-formed range: logits
    +-100 (opacity exactly 1 and 0), log-scales 89 (inf), -90 (subnormal) and
    -104 (0), NaN, zero rotations, NaN positions.  The product's loader
    equals the oracle's restatement (and the reference's own loader where it
    was built) bit for bit; the crop drops the NaN positions."""
    from gaussian_splat_amd import InstancedSplatRenderer, Options, PLYLoader
    from gaussian_splat_amd import scene as S
    raw = S.synthetic_raw(256, seed=47)
    raw.opacity_logit[0:8:2], raw.opacity_logit[1:8:2] = 100.0, -100.0
    raw.log_scale[8:12, 0] = [89.0, -90.0, -104.0, np.nan]
    raw.log_scale[12:16] = [89.0, -90.0, -104.0]
    raw.opacity_logit[16:18] = np.nan
    raw.f_dc[18:20, 1] = np.nan
    raw.f_rest[20:22, 5] = np.nan
    raw.rot[22:26] = 0.0
    raw.rot[26:28, 2] = np.nan
    raw.pos[28:31, 0] = np.nan
    raw.pos[31:33] = np.nan
    nanpos = 5
    p = S.write_ply(tmp_path / "zoo.ply", raw)
    ok, a = PLYLoader.load(p)
    ok2, b = O.ply_load(p)
    assert ok and ok2 and a.shape == b.shape == (256, 62)
    assert same_frame(a, b) == (0, 0)
    if O.ref_available():
        ok3, c = O.ref_ply_load(p)
        assert ok3 and same_frame(a, c) == (0, 0)
    assert a[0, 9] == 1.0 and a[1, 9] == 0.0
    assert np.isinf(a[8, 10]) and 0 < a[9, 10] < np.finfo(np.float32).tiny and a[10, 10] == 0.0 and np.isnan(a[11, 10])
    assert np.isnan(a[16, 9]) and np.isnan(a[28, 0])
    keep = O.crop(b)
    assert len(keep) == 256 - nanpos and not np.isnan(b[keep, 0:3]).any()
    assert set(range(256)) - set(keep.tolist()) == set(range(28, 33))
    assert InstancedSplatRenderer(str(p)).getPointCount() == 256 - nanpos
    # a crop-free load keeps them (culled every frame)
    assert InstancedSplatRenderer(str(p), Options(crop=False)).getPointCount() == 256


def test_same_records():
    rec = np.zeros(4, O.RECORD_DTYPE)
    rec["opacity"][1] = np.nan
    other = rec.copy()
    other["opacity"][1] = -np.float32(np.nan)
    assert same_records(other, rec) == (0, 0)
    other["rect_hi"][2] = 1
    other["cx"][3] = 1.0
    assert same_records(other, rec) == (0, 2)
    other["g"][0] = np.nan
    assert same_records(other, rec) == (1, 2)
