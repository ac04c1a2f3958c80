"""gs_render_contrib on the GPU: the colour frame and each splat's quantised blend weight
totals (sum, count, max), against the CPU oracle for equality
(tests/contrib_ref.py).

Shapes: 333 x 211 runs composite_contrib_kernel (77 bins; ragged right and bottom
edges), 1037 x 531 composite_strip_contrib_kernel (561 bins; the right tile wholly
outside the frame, 3 of 16 rows in the last bins); 1024 x 512 / 1025 x 512 are the last
tile-kernel and first strip-kernel bin counts (512 / 513); 17 x 9 and 1 x 1 the smallest
frames.  The scenes, views and cached projections are test_gpu_depth_output.py's; the
reference's fragments are computed once per (scene, shape, rule) and left unchanged."""
import functools

import numpy as np
import pytest

from conftest import orbit_views
from contrib_ref import contrib_fragments, contrib_totals
from depth_ref import depth_from_projection, project_zf
from features_ref import features_from_projection
from test_gpu_depth_output import STRIP_MIN_BINS, _bins, _bits, _hip, _projection, _scene
from test_gpu_frame_shapes import _cat, _splats_at

pytestmark = pytest.mark.gpu

SHAPES = [(333, 211), (1037, 531)]
MODES = ["tile", "live50"]
SENT64 = 0x5A5A5A5A5A5A5A5A
SENT32 = 0x5A5A5A5A
GUARD = 64


def _key(W, H, sh=0):
    """The parity scenes: test_gpu_features.py's 40 000 splats at 333 x 211, 4 000 at 1037 x 531."""
    return ((40000 if (W, H) == (333, 211) else 4000, 7, sh, W / H, 3.0), W, H, sh)


STACK_FRONT, STACK_BACK = 250, 550


@functools.lru_cache(maxsize=None)
def _stacked(W, H):
    """The 4 000-splat scene plus 800 splats stacked at the centre of one bin (the bin at
    (512, 256) of 1037 x 531, at (160, 96) of 333 x 211): 250 low-opacity splats about 8 px
    wide, first in the composite's order (largest zF first), which saturate the middle of the
    bin only after a good part of a batch of them, and 550 small ones over the middle, later in
    that order, which get nothing.  The bin's list is more than three 256-record batches long.
    (scene, V, P, projection)."""
    sc = _scene(4000, 7, 0, W / H, 3.0)
    V, P = orbit_views(W, H, 1)[0]
    cx, cy = ((528.0, 272.0) if (W, H) == (1037, 531) else (176.0, 112.0))
    rng = np.random.default_rng(12)
    nf, nb = STACK_FRONT, STACK_BACK
    front = _splats_at(V, P, W, H, cx + rng.uniform(-2.0, 2.0, nf), cy + rng.uniform(-2.0, 2.0, nf), rng, sigma_px=8.0,
                       depths=(9.5,))
    front.opacity = rng.uniform(0.04, 0.08, nf).astype(np.float32)
    back = _splats_at(V, P, W, H, cx + rng.uniform(-2.0, 2.0, nb), cy + rng.uniform(-2.0, 2.0, nb), rng, sigma_px=0.8,
                      depths=(2.0,))
    both = _cat(sc, front, back)
    return both, V, P, project_zf(both, V, P, W, H, 0)


SMALL = (600, 5, 0, 1.0, 2.0)  # the covering scene of the frames of one bin (every splat shares their tiles: a set each)


@functools.lru_cache(maxsize=None)
def _small_half(W, H):
    """The small covering scene's splats left of the world's x = -0.5 plane, as _half_scene."""
    from gaussian_splat_amd.api import Scene
    sc = _scene(SMALL[0], SMALL[1], 0, max(W / H, 1.0), SMALL[4])
    keep = sc.pos[:, 0] < -0.5
    sc = Scene(pos=sc.pos[keep], rot=sc.rot[keep], scale=sc.scale[keep], opacity=sc.opacity[keep], color=sc.color[keep])
    V, P = orbit_views(W, H, 1)[0]
    return sc, V, P, project_zf(sc, V, P, W, H, 0)


@functools.lru_cache(maxsize=None)
def _ref(key, mode):
    """(scene, V, P, fragments, oracle colour frame, info, N) of a (scene key, W, H, sh) and rule."""
    skey, W, H, sh = key
    if skey == "stacked":
        sc, V, P, proj = _stacked(W, H)
    elif skey == "small_half":
        sc, V, P, proj = _small_half(W, H)
    else:
        sc, V, P, proj = _projection(key)
    fr = contrib_fragments(sc, V, P, W, H, mode, sh, proj)
    return sc, V, P, fr, fr[3], fr[4], proj[0].shape[0]


def _np(sum_, count, max_):
    """The three device tensors as the uint64 / uint32 arrays they hold."""
    return (sum_.cpu().numpy().view(np.uint64), count.cpu().numpy().view(np.uint32), max_.cpu().numpy().view(np.uint32))


def _same(got, want, what=None):
    for name, g, w in zip(("sum", "count", "max"), got, want):
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        assert bad.size == 0, (what, name, bad.size, int(bad[0]), int(g[bad[0]]), int(w[bad[0]]))


def _dev_mask(mask):
    import torch
    return None if mask is None else torch.tensor(np.asarray(mask), dtype=torch.uint8, device="cuda:0")


def _masks(W, H):
    rect = np.zeros((H, W), np.uint8)
    rect[H // 5:H - H // 3, W // 4:W - W // 7] = 1
    return {"random": (np.random.default_rng(21).random((H, W)) < 0.5).astype(np.uint8), "rect": rect,
            "ones": np.ones((H, W), np.uint8), "zeros": np.zeros((H, W), np.uint8)}


# ------------------------------------------------------------------ 1. parity

PARITY = ([(W, H, m, c, fif, 0) for (W, H) in SHAPES for m in MODES for c in (False, True) for fif in (1, 2)] +
          [(1037, 531, "tile", True, 2, 3)])


@pytest.mark.parametrize("W,H,mode,cut,fif,sh", PARITY)
def test_contrib_parity(built, W, H, mode, cut, fif, sh):
    """Four frames under a still camera: sum, count and max equal contrib_ref on the first and
    the last frame; colour equals the oracle's and gs_render's on a second (whole-list) handle
    on every frame; every frame is a whole-list frame whatever depth_split says; the
    composite's algorithmic bytes follow the documented identity."""
    assert (_bins(W, H) > STRIP_MIN_BINS) == ((W, H) == (1037, 531))
    sc, V, P, fr, cref, info, N = _ref(_key(W, H, sh), mode)
    want = contrib_totals(fr, N)
    assert (cref[..., 3] > 0).mean() > 0.5 and (want[1] > 0).mean() > 0.5
    r = _hip(sc, mode=mode, depth_split=cut, sh_degree=sh, frames_in_flight=fif)
    plain = _hip(sc, mode=mode, depth_split=False, sh_degree=sh)
    for k in range(4):
        rgba, s, c, m = r.render_contrib(V, P, W, H)
        rgba = rgba.cpu().numpy()
        st = r.last_stats()
        assert _bits(rgba, plain.render_host(V, P, W, H)) == 0, k
        assert _bits(rgba, cref) == 0, k
        if k in (0, 3):
            _same(_np(s, c, m), want, k)
        assert st["cut_frame"] == 0, (k, st)
    print(f"{W}x{H} {mode} cuts {cut} fif {fif} sh {sh}: sets {info['sets']} pairs {st['pairs']} "
          f"fetched {st['records_fetched']} splats with weight {int((want[1] > 0).sum())} of {N}")
    # a contrib frame's algorithmic composite bytes: its pass reads the range words and the fetched
    # records again (B0), and the mask where there is one; the scatter is not counted
    ps = plain.last_stats()
    assert ps["cut_frame"] == 0 and st["records_fetched"] == ps["records_fetched"] > 0
    B0 = ps["bytes_composite"] - 16 * W * H
    assert st["bytes_composite"] - ps["bytes_composite"] == B0
    r.render_contrib(V, P, W, H, mask=_dev_mask(_masks(W, H)["random"]))
    assert r.last_stats()["bytes_composite"] - ps["bytes_composite"] == B0 + W * H


# -------------------------------------------------------------- 2. long lists

@pytest.mark.parametrize("skey,W,H,mode", [((12000, 7, 0, 333 / 211, 12.0), 333, 211, "tile"),
                                           ("stacked", 333, 211, "live50"), ("stacked", 1037, 531, "tile")])
def test_contrib_long_lists(built, skey, W, H, mode):
    """Lists of more than two 256-record batches, pixels that saturate (the early outs) and
    splats behind them that get nothing: the pruning case.  Tile kernel: a dense scene under
    the tile rule, and the stack under the live50 rule (whose oracle is ten times slower on
    the dense frame); strip kernel: the stack."""
    sc, V, P, fr, cref, info, N = _ref((skey, W, H, 0), mode)
    assert info["longest_tile_list"] >= 513, info
    sat = cref[..., 3] >= np.float32(1.0) - np.float32(0.01)  # both rules stop at T = 0.01 (fp32)
    if skey == "stacked":  # (the middle of the stack's bin)
        cx, cy = (528, 272) if W == 1037 else (176, 112)
        assert sat[cy - 4:cy + 4, cx - 4:cx + 4].all() and not sat[cy - 16:cy + 16, cx - 16:cx + 16].all()
    else:
        assert sat.mean() > 0.25
    want = contrib_totals(fr, N)
    assert (want[1] == 0).mean() > 0.1, (want[1] == 0).mean()
    print(f"{W}x{H} {mode}: longest tile list {info['longest_tile_list']}, sets {info['sets']}, "
          f"saturated {sat.mean():.3f}, splats with nothing {(want[1] == 0).mean():.3f}")
    r = _hip(sc, mode=mode)
    for k in range(2):
        rgba, s, c, m = r.render_contrib(V, P, W, H)
        assert _bits(rgba.cpu().numpy(), cref) == 0, k
        _same(_np(s, c, m), want, k)


# -------------------------------------------------------------------- 3. mask

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H", SHAPES)
def test_contrib_mask(built, W, H, mode):
    """A seeded random mask, a rectangle, all ones and all zeros (uint8), and the random one as
    torch.bool: totals over the masked pixels only; all ones is the NULL mask, all zeros gives
    zeros; the colour frame is the same in every case."""
    import torch
    sc, V, P, fr, cref, info, N = _ref(_key(W, H), mode)
    r = _hip(sc, mode=mode)
    whole = contrib_totals(fr, N)
    for name, mask in _masks(W, H).items():
        want = contrib_totals(fr, N, mask)
        rgba, s, c, m = r.render_contrib(V, P, W, H, mask=_dev_mask(mask))
        assert _bits(rgba.cpu().numpy(), cref) == 0, name
        got = _np(s, c, m)
        _same(got, want, name)
        if name == "ones":
            _same(got, whole, name)
        elif name == "zeros":
            assert not got[0].any() and not got[1].any() and not got[2].any()
        else:
            assert 0 < int(want[0].sum()) < int(whole[0].sum())
    mb = torch.tensor(_masks(W, H)["random"] != 0, device="cuda:0")
    assert mb.dtype == torch.bool
    _same(_np(*r.render_contrib(V, P, W, H, mask=mb)[1:]), contrib_totals(fr, N, _masks(W, H)["random"]), "bool")


# -------------------------------------------------------------- 4. accumulate

@pytest.mark.parametrize("W,H", SHAPES)
def test_contrib_accumulate(built, W, H):
    """Three orbit views accumulated into zeroed arrays are the element-wise sum / sum / max of
    the three frames' references; accumulated into sentinel-filled arrays, the entries of splats
    the reference gives nothing keep the sentinel; accumulate=False writes every entry."""
    import torch
    sc = _scene(6000 if (W, H) == (333, 211) else 4000, 7, 0, W / H, 8.0 if (W, H) == (333, 211) else 3.0)
    N = sc.pos.shape[0]
    views = orbit_views(W, H, 3)
    refs = []
    for V, P in views:
        fr = contrib_fragments(sc, V, P, W, H, "tile", 0, project_zf(sc, V, P, W, H, 0))
        refs.append(contrib_totals(fr, N))
    r = _hip(sc, frames_in_flight=2)
    s = torch.zeros(N, dtype=torch.int64, device="cuda:0")
    c = torch.zeros(N, dtype=torch.int32, device="cuda:0")
    m = torch.zeros(N, dtype=torch.int32, device="cuda:0")
    for V, P in views:
        out = r.render_contrib(V, P, W, H, sum=s, count=c, max=m, accumulate=True)
        assert out[1] is s and out[2] is c and out[3] is m
    tot = (refs[0][0] + refs[1][0] + refs[2][0], refs[0][1] + refs[1][1] + refs[2][1],
           np.maximum(np.maximum(refs[0][2], refs[1][2]), refs[2][2]))
    _same(_np(s, c, m), tot, "accumulated")
    # sentinels: a splat without a contribution is not touched
    s.fill_(1 << 40)
    c.fill_(7)
    m.fill_(1 << 25)  # (above every q)
    V, P = views[2]
    r.render_contrib(V, P, W, H, sum=s, count=c, max=m, accumulate=True)
    none = refs[2][1] == 0
    if (W, H) == (333, 211):
        assert none.sum() > 100
    _same(_np(s, c, m), (refs[2][0] + np.uint64(1 << 40), refs[2][1] + np.uint32(7), np.full(N, 1 << 25, np.uint32)),
          "sentinel")
    m.fill_(0)
    r.render_contrib(V, P, W, H, sum=s, count=c, max=m, accumulate=True)
    assert (_np(s, c, m)[2] == refs[2][2]).all() and (_np(s, c, m)[2][none] == 0).all()
    # accumulate=False: every entry is written, zeros included
    s.fill_(SENT64)
    c.fill_(SENT32)
    m.fill_(SENT32)
    r.render_contrib(V, P, W, H, sum=s, count=c, max=m)
    _same(_np(s, c, m), refs[2], "overwritten")


# ------------------------------------------------------------------ 5. bounds

class GuardedContrib:
    """The three device arrays of n entries, each between two guards of GUARD entries, all
    filled with a sentinel."""

    def __init__(self, n):
        import torch
        self.n = n
        self.bs = torch.full((n + 2 * GUARD,), SENT64, dtype=torch.int64, device="cuda:0")
        self.bc = torch.full((n + 2 * GUARD,), SENT32, dtype=torch.int32, device="cuda:0")
        self.bm = torch.full((n + 2 * GUARD,), SENT32, dtype=torch.int32, device="cuda:0")
        self.sum, self.count, self.max = (b[GUARD:GUARD + n] for b in (self.bs, self.bc, self.bm))
        assert self.sum.data_ptr() % 8 == 0 and self.count.data_ptr() % 4 == 0

    def arrays(self, written=True):
        import torch
        torch.cuda.synchronize()
        out = []
        for b, sent, dt in ((self.bs, SENT64, np.uint64), (self.bc, SENT32, np.uint32), (self.bm, SENT32, np.uint32)):
            raw = b.cpu().numpy().view(dt)
            assert (raw[:GUARD] == sent).all() and (raw[GUARD + self.n:] == sent).all(), "guard entries written"
            mid = raw[GUARD:GUARD + self.n]
            if written:
                assert not (mid == sent).any(), "entries never written"
            out.append(mid.copy())
        return tuple(out)


@pytest.mark.parametrize("W,H", [(1, 1), (17, 9), (1024, 512), (1025, 512)])
def test_contrib_bounds(built, W, H):
    """Nothing outside the N entries of each array is written and every entry of them is, on
    the half-empty scene and on a covering scene (20 000 splats; 600 in the frames of one bin,
    where every splat needs a set of its own in the reference)."""
    assert (_bins(W, H) > STRIP_MIN_BINS) == ((W, H) == (1025, 512))
    scenes = ("half", (20000, 5, 0, max(W / H, 1.0), 2.0))
    if _bins(W, H) == 1:
        scenes = ("small_half", (SMALL[0], SMALL[1], 0, max(W / H, 1.0), SMALL[4]))
    for skey in scenes:
        sc, V, P, fr, cref, info, N = _ref((skey, W, H, 0), "tile")
        want = contrib_totals(fr, N)
        if W > 1:
            assert (want[1] > 0).any()
        r = _hip(sc)
        for k in range(2):
            g = GuardedContrib(N)
            rgba = r.render_contrib(V, P, W, H, sum=g.sum, count=g.count, max=g.max)[0]
            _same(g.arrays(), want, (skey, k))
            assert _bits(rgba.cpu().numpy(), cref) == 0, (skey, k)


def test_contrib_empty_scene(built):
    """A scene of 0 splats: NULL arrays are accepted and the frame is empty."""
    import ctypes as C
    from gaussian_splat_amd._lib import check, lib
    from gaussian_splat_amd.api import Scene, _mat16
    z = lambda *s: np.zeros(s, np.float32)
    r = _hip(Scene(pos=z(0, 3), rot=z(0, 4), scale=z(0, 3), opacity=z(0), color=z(0, 3)))
    assert r.getPointCount() == 0
    W, H = 33, 17
    V, P = orbit_views(W, H, 1)[0]
    out = np.full((H, W, 4), np.nan, np.float32)
    check(lib().gs_render_contrib(r._h, _mat16(V), _mat16(P), W, H, None, out.ctypes.data, None, None, None, 0, 0,
                                  None), "gs_render_contrib")
    assert (out.view(np.uint32) == 0).all()
    rgba, s, c, m = r.render_contrib(V, P, W, H)
    assert s.numel() == 0 and c.numel() == 0 and m.numel() == 0 and not rgba.cpu().numpy().any()


# --------------------------------------------------- 6. host path and sequences

@pytest.mark.parametrize("W,H", SHAPES)
def test_contrib_host_path(built, W, H):
    """render_contrib_host equals the device path and the reference, with and without a mask
    and accumulate."""
    sc, V, P, fr, cref, info, N = _ref(_key(W, H), "tile")
    mask = _masks(W, H)["random"]
    want, wantm = contrib_totals(fr, N), contrib_totals(fr, N, mask)
    r = _hip(sc)
    for k in range(2):
        ch, hs, hc, hm = r.render_contrib_host(V, P, W, H)
        cd, ds, dc, dm = r.render_contrib(V, P, W, H)
        assert hs.dtype == np.uint64 and hc.dtype == np.uint32 and hm.dtype == np.uint32
        assert _bits(ch, cd.cpu().numpy()) == 0 and _bits(ch, cref) == 0, k
        _same((hs, hc, hm), want, k)
        _same(_np(ds, dc, dm), want, k)
    hs, hc, hm = np.full(N, 5, np.uint64), np.full(N, 6, np.uint32), np.full(N, 1 << 25, np.uint32)
    out = r.render_contrib_host(V, P, W, H, mask=mask, sum=hs, count=hc, max=hm, accumulate=True)
    assert out[1] is hs and _bits(out[0], cref) == 0
    _same((hs, hc, hm), (wantm[0] + np.uint64(5), wantm[1] + np.uint32(6), np.full(N, 1 << 25, np.uint32)), "acc")
    hm[:] = 0
    r.render_contrib_host(V, P, W, H, mask=mask.astype(bool), sum=hs, count=hc, max=hm, accumulate=True)
    _same((hs, hc, hm), (wantm[0] * np.uint64(2) + np.uint64(5), wantm[1] * np.uint32(2) + np.uint32(6), wantm[2]),
          "acc twice")
    _same(r.render_contrib_host(V, P, W, H, mask=mask)[1:], wantm, "host mask")


def test_contrib_sequence_on_one_handle(built):
    """colour, contrib, depth, contrib with a mask, features, colour, colour on one handle with
    depth cuts and two frames in flight, into reused tensors: every output equals its reference;
    contrib and feature frames are whole-list frames, the colour and depth frames around them
    are depth-cut frames again (their buffer set learns its cuts anew, §2.12)."""
    import torch
    W, H, K = 1037, 531, 4
    sc, V, P, fr, cref, info, N = _ref(_key(W, H), "tile")
    proj = _projection(_key(W, H))[3]
    mask = _masks(W, H)["rect"]
    want, wantm = contrib_totals(fr, N), contrib_totals(fr, N, mask)
    dref, _ = depth_from_projection(sc, V, P, W, H, "tile", 0, proj)
    f = np.random.default_rng(5).standard_normal((N, K)).astype(np.float32)
    fref, _ = features_from_projection(sc, V, P, W, H, "tile", 0, proj, f)
    r = _hip(sc, depth_split=True, frames_in_flight=2)
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    depth = torch.empty((H, W), dtype=torch.float32, device="cuda:0")
    fd = torch.tensor(f, device="cuda:0")
    got = []
    for step in ("colour", "contrib", "depth", "mask", "features", "colour", "colour", "colour", "contrib", "colour"):
        extra = None
        if step == "colour":
            r.render(V, P, W, H, out=out)
        elif step == "depth":
            r.render_depth(V, P, W, H, out=out, depth=depth)
            extra = depth.clone()
        elif step == "features":
            extra = r.render_features(V, P, W, H, fd, out=out)[1]
        else:
            extra = r.render_contrib(V, P, W, H, mask=_dev_mask(mask) if step == "mask" else None, out=out)[1:]
        got.append((step, out.clone(), extra, r.last_stats()["cut_frame"]))
    torch.cuda.synchronize()
    for j, (step, c, extra, cutf) in enumerate(got):
        assert _bits(c.cpu().numpy(), cref) == 0, (j, step)
        assert cutf == (1 if step in ("colour", "depth") else 0), (j, step, cutf)
        if step == "depth":
            assert _bits(extra.cpu().numpy(), dref) == 0, j
        elif step == "features":
            assert _bits(extra.cpu().numpy(), fref) == 0, j
        elif step in ("contrib", "mask"):
            _same(_np(*extra), wantm if step == "mask" else want, (j, step))


# ------------------------------------------------------------- 7. unsupported

@pytest.mark.parametrize("opts", [dict(cap=32), dict(mode="mlab"), dict(shard=True)])
def test_contrib_unsupported(built, opts):
    """cap > 0, MLAB and a handle configured as one rank of two: GS_ERR_UNSUPPORTED, and the
    output buffers stay untouched."""
    import torch
    from gaussian_splat_amd._lib import GsError, check, lib
    W, H = 333, 211
    opts = dict(opts)
    shard = opts.pop("shard", False)
    sc = _scene(40000, 7, 0, W / H, 3.0)
    N = sc.pos.shape[0]
    V, P = orbit_views(W, H, 1)[0]
    r = _hip(sc, **opts)
    if shard:
        check(lib().gs_shard_configure(r._h, 0, 2, 0), "gs_shard_configure")
    g = GuardedContrib(N)
    out = torch.full((H, W, 4), -3.0, dtype=torch.float32, device="cuda:0")
    with pytest.raises(GsError) as e:
        r.render_contrib(V, P, W, H, out=out, sum=g.sum, count=g.count, max=g.max)
    assert e.value.status == 7 and "GS_ERR_UNSUPPORTED" in str(e.value) and "gs_render_contrib" in str(e.value)
    got = g.arrays(written=False)
    assert (got[0] == SENT64).all() and (got[1] == SENT32).all() and (got[2] == SENT32).all()
    assert (out.cpu().numpy() == -3.0).all()
    hs, hc, hm = np.full(N, 9, np.uint64), np.full(N, 9, np.uint32), np.full(N, 9, np.uint32)
    with pytest.raises(GsError) as e:
        r.render_contrib_host(V, P, W, H, sum=hs, count=hc, max=hm)
    assert e.value.status == 7 and (hs == 9).all() and (hc == 9).all() and (hm == 9).all()
    if shard:  # back to one rank: the call works again
        check(lib().gs_shard_configure(r._h, 0, 1, 0), "gs_shard_configure")
        fr = _ref(_key(W, H), "tile")[3]
        _same(r.render_contrib_host(V, P, W, H)[1:], contrib_totals(fr, N), "unsharded")
