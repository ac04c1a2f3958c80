"""gs_render_features on the GPU: colour and K per-splat feature channels composited per
pixel, against the CPU oracle bit for bit (tests/features_ref.py).

Shapes: 333 x 211 runs composite_feat_kernel (77 bins; ragged right and bottom edges),
1037 x 531 composite_strip_feat_kernel (561 bins; the right tile wholly outside the
frame, 3 of 16 rows in the last bins); 1024 x 512 / 1025 x 512 are the last tile-kernel
and first strip-kernel bin counts (512 / 513); 17 x 9 and 1 x 1 the smallest frames.
The scenes, views and cached projections are test_gpu_depth_output.py's.  Features are
seeded standard-normal float32 unless a test says otherwise."""
import functools

import numpy as np
import pytest

from conftest import orbit_views
from depth_ref import project_zf
from features_ref import features_from_projection
from test_gpu_depth_output import SENT_F32, STRIP_MIN_BINS, _bins, _bits, _half_scene, _hip, _projection, _scene

pytestmark = pytest.mark.gpu

SHAPES = [(333, 211), (1037, 531)]
MODES = ["tile", "live50"]


@functools.lru_cache(maxsize=None)
def _features(n, K, seed=1):
    f = np.random.default_rng(seed).standard_normal((n, K)).astype(np.float32)
    f.setflags(write=False)
    return f


def _dev(a):
    import torch
    return torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda:0")  # (a copy: the cached arrays are read-only)


@functools.lru_cache(maxsize=None)
def _ref(key, mode, K, seed=1):
    """(scene, V, P, features, features_ref, oracle colour frame), computed once and left unchanged."""
    skey, W, H, sh = key
    sc, V, P, proj = _projection(key)
    f = _features(sc.pos.shape[0], K, seed)
    fref, colour = features_from_projection(sc, V, P, W, H, mode, sh, proj, f)
    return sc, V, P, f, fref, colour


def _passes(K):
    return (K + 3) // 4


# ------------------------------------------------------------------ 1. parity

PARITY = ([(W, H, m, c, 0, 3.0, K) for (W, H) in SHAPES for m in MODES for c in (False, True)
           for K in (1, 3, 4, 5, 8, 9)] +  # 1, 1, 1, 2, 2 and 3 passes; tails of 1 and 3 channels
          # splats x12: lists of many 256-record batches (the software pipeline's prefetched
          # values) and pixels that saturate (the early outs)
          [(W, H, m, True, 0, 12.0, 5) for (W, H) in SHAPES for m in MODES] +
          [(333, 211, "tile", True, 3, 3.0, 4), (1037, 531, "live50", False, 3, 3.0, 4)] +
          [(333, 211, m, True, 0, 3.0, 64) for m in MODES])


@pytest.mark.parametrize("W,H,mode,cut,sh,scale,K", PARITY)
def test_features_parity(built, W, H, mode, cut, sh, scale, K):
    """Four frames under a still camera: features equal features_ref on the first and the
    last frame; colour equals the oracle's and gs_render's on a second (whole-list) handle
    on every frame; every frame is a whole-list frame whatever depth_split says; the
    composite's algorithmic bytes follow the documented identity."""
    assert (_bins(W, H) > STRIP_MIN_BINS) == ((W, H) == (1037, 531))
    sc, V, P, f, fref, cref = _ref(((40000, 7, sh, W / H, scale), W, H, sh), mode, K)
    if scale > 3.0:  # both rules stop at T = 0.01: saturated pixels have alpha >= 1 - 0.01 (fp32)
        assert (cref[..., 3] >= np.float32(1.0) - np.float32(0.01)).mean() > 0.25
    assert (cref[..., 3] > 0).mean() > 0.5  # the frame is mostly covered
    r = _hip(sc, mode=mode, depth_split=cut, sh_degree=sh)
    plain = _hip(sc, mode=mode, depth_split=False, sh_degree=sh)
    fd = _dev(f)
    for k in range(4):
        rgba, feats = r.render_features(V, P, W, H, fd)
        rgba, feats = rgba.cpu().numpy(), feats.cpu().numpy()
        st = r.last_stats()
        assert feats.shape == (H, W, K)
        assert _bits(rgba, plain.render_host(V, P, W, H)) == 0, k
        assert _bits(rgba, cref) == 0, k
        if k in (0, 3):
            assert _bits(feats, fref) == 0, (k, _bits(feats, fref))
        assert st["cut_frame"] == 0, (k, st)
    print(f"{W}x{H} {mode} cuts {cut} sh {sh} x{scale} K {K}: pairs {st['pairs']} fetched {st['records_fetched']}")
    # a feature frame's algorithmic composite bytes: every pass reads the range words and the
    # fetched records again (B0), 4 K bytes of values per fetched record, and the feature image
    ps = plain.last_stats()
    assert ps["cut_frame"] == 0
    R = ps["records_fetched"]
    assert st["records_fetched"] == R > 0
    B0 = ps["bytes_composite"] - 16 * W * H
    assert st["bytes_composite"] - ps["bytes_composite"] == _passes(K) * B0 + 4 * K * R + 4 * K * W * H


# ------------------------------------------------------------------ 2. bounds

class GuardedFeatures:
    """A device feature image between two guards of one frame row (rounded up to 4
    words, so the image is 16-B aligned), all filled with a NaN sentinel."""

    def __init__(self, W, H, K):
        import torch
        self.W, self.H, self.K, self.n, self.g = W, H, K, W * H * K, (W * K + 3) // 4 * 4
        self.buf = torch.full((self.n + 2 * self.g,), SENT_F32, dtype=torch.int32, device="cuda:0")
        self.out = self.buf[self.g:self.g + self.n].view(torch.float32).view(H, W, K)
        assert self.out.is_contiguous() and self.out.data_ptr() % 16 == 0

    def frame(self):
        import torch
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy().view(np.uint32)
        g, n = self.g, self.n
        assert not (raw[:g] != SENT_F32).any() and not (raw[g + n:] != SENT_F32).any(), "guard words written"
        mid = raw[g:g + n]
        stale = np.nonzero(mid == SENT_F32)[0]
        assert stale.size == 0, (f"{stale.size} feature words never written, first at pixel "
                                 f"({int(stale[0]) // self.K % self.W}, {int(stale[0]) // self.K // self.W}) "
                                 f"channel {int(stale[0]) % self.K}")
        return mid.view(np.float32).reshape(self.H, self.W, self.K).copy()


@pytest.mark.parametrize("K", [5, 4])
@pytest.mark.parametrize("W,H", [(1, 1), (17, 9), (1024, 512), (1025, 512)])
def test_features_bounds(built, W, H, K):
    """Nothing is written outside the feature image and every word of it is, empty pixels
    (and empty bins) with exactly 0.0 in every channel; then the same shape with the frame
    covered (at 1 x 1 the only pixel is empty in the first scene).  K = 5: dword stores,
    the last pixel's tail store is the one that would cross the end; K = 4: 16-B stores."""
    assert (_bins(W, H) > STRIP_MIN_BINS) == ((W, H) == (1025, 512))
    for skey in ("half", (20000, 5, 0, max(W / H, 1.0), 2.0)):
        sc, V, P, f, fref, cref = _ref((skey, W, H, 0), "tile", K)
        empty = cref[..., 3] == 0
        if skey == "half":
            assert empty.any() and (fref[empty] == 0.0).all()
        else:
            assert (~empty).any()
        r = _hip(sc)
        fd = _dev(f)
        for k in range(2):
            g = GuardedFeatures(W, H, K)
            rgba, _ = r.render_features(V, P, W, H, fd, out_features=g.out)
            feats = g.frame()
            assert _bits(feats, fref) == 0 and _bits(rgba.cpu().numpy(), cref) == 0, (skey, k)
            assert (feats[empty].view(np.uint32) == 0).all()  # exactly +0.0


# --------------------------------------------------------------- 3. alignment

@pytest.mark.parametrize("K,fin,fout", [(4, 1, 1), (8, 1, 1), (4, 0, 0), (4, 0, 1), (4, 1, 0)])
@pytest.mark.parametrize("W,H", SHAPES)
def test_features_alignment(built, W, H, K, fin, fout):
    """features and out_features as views one float into larger tensors (4-B aligned, not
    16-B: dword gathers and stores although K % 4 == 0), both 16-B aligned (16-B gathers
    and stores), and one of each; the words around the image stay untouched."""
    import torch
    sc, V, P, f, fref, cref = _ref(((40000, 7, 0, W / H, 3.0), W, H, 0), "tile", K)
    N = f.shape[0]
    fbuf = torch.zeros((N * K + 8,), dtype=torch.float32, device="cuda:0")
    fv = fbuf[fin:fin + N * K].view(N, K)
    fv.copy_(_dev(f))
    obuf = torch.full((H * W * K + 8,), SENT_F32, dtype=torch.int32, device="cuda:0")
    ov = obuf[fout:fout + H * W * K].view(torch.float32).view(H, W, K)
    assert fv.data_ptr() % 16 == 4 * fin and ov.data_ptr() % 16 == 4 * fout
    r = _hip(sc)
    rgba, feats = r.render_features(V, P, W, H, fv, out_features=ov)
    assert feats.data_ptr() == ov.data_ptr()
    assert _bits(feats.cpu().numpy(), fref) == 0 and _bits(rgba.cpu().numpy(), cref) == 0
    raw = obuf.cpu().numpy().view(np.uint32)
    assert (raw[:fout] == SENT_F32).all() and (raw[fout + H * W * K:] == SENT_F32).all()


# -------------------------------------------------------------- 4. unused rows

@functools.lru_cache(maxsize=None)
def _near(W, H):
    """The default camera pulled in to distance 2.0 on the bounds tests' covering scene: most
    splats are culled.  (scene, V, P, projection), computed once."""
    from gaussian_splat_amd.api import default_camera
    sc = _scene(20000, 5, 0, max(W / H, 1.0), 2.0)
    cam = default_camera(W, H)
    cam.setDistance(2.0)
    V, P = cam.getViewMatrix(), cam.getProjectionMatrix()
    return sc, V, P, project_zf(sc, V, P, W, H, 0)


@pytest.mark.parametrize("K", [5, 4])
@pytest.mark.parametrize("W,H", SHAPES)
def test_features_unused_rows(built, W, H, K):
    """Rows of splats that reach no bin list are never used: with NaN written into exactly
    the rows the oracle culls, the images equal the reference of the clean matrix."""
    sc, V, P, proj = _near(W, H)
    culled = proj[2] == 0
    print(f"{W}x{H}: {int(culled.sum())} of {culled.size} splats culled")
    assert culled.sum() >= 1000 and (~culled).sum() >= 1000
    f = _features(culled.size, K, seed=2)
    fref, cref = features_from_projection(sc, V, P, W, H, "tile", 0, proj, f)
    assert (cref[..., 3] > 0).any() and not np.isnan(fref).any()
    dirty = f.copy()
    dirty[culled] = np.nan
    r = _hip(sc)
    rgba, feats = r.render_features(V, P, W, H, _dev(dirty))
    feats = feats.cpu().numpy()
    assert not np.isnan(feats).any()
    assert _bits(feats, fref) == 0 and _bits(rgba.cpu().numpy(), cref) == 0


# --------------------------------------------------------- 5. depth equivalence

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H", SHAPES)
def test_features_one_channel_of_zf_is_render_depth(built, W, H, mode):
    """Depth is the case K = 1, f = zF: with the oracle's zF column, the feature image
    equals render_depth's depth image bit for bit."""
    sc, V, P, proj = _projection(((40000, 7, 0, W / H, 3.0), W, H, 0))
    zf = np.ascontiguousarray(proj[3].reshape(-1, 1))
    r = _hip(sc, mode=mode)
    rgba_d, depth = r.render_depth(V, P, W, H)
    rgba_f, feats = r.render_features(V, P, W, H, _dev(zf))
    depth, feats = depth.cpu().numpy(), feats.cpu().numpy()
    assert (depth != 0).any()
    assert _bits(feats[..., 0], depth) == 0 and _bits(rgba_f.cpu().numpy(), rgba_d.cpu().numpy()) == 0


# ---------------------------------------------------------- 6. non-finite values

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H", SHAPES)
def test_features_non_finite_values(built, W, H, mode):
    """inf, -inf, NaN and 1e30 in channel 2 of K = 4, in 400 rows of visible splats: they
    propagate into that channel and into nothing else (termination depends on T alone).
    All four channels equal the reference, NaN words compared by their bits too; colour is
    unchanged."""
    key = ((40000, 7, 0, W / H, 3.0), W, H, 0)
    sc, V, P, proj = _projection(key)
    _, _, _, f0, fref0, cref = _ref(key, mode, 4)
    vis = np.nonzero(proj[2] > 0)[0]
    rows = np.random.default_rng(6).choice(vis, 400, replace=False)
    f = f0.copy()
    f[rows, 2] = np.tile(np.array([np.inf, -np.inf, np.nan, 1e30], np.float32), 100)
    fref, _ = features_from_projection(sc, V, P, W, H, mode, 0, proj, f)
    assert np.isnan(fref[..., 2]).any() and np.isinf(fref[..., 2]).any()
    for c in (0, 1, 3):
        assert np.isfinite(fref[..., c]).all() and _bits(fref[..., c], fref0[..., c]) == 0
    r = _hip(sc, mode=mode)
    rgba, feats = r.render_features(V, P, W, H, _dev(f))
    feats = feats.cpu().numpy()
    a, b = feats.view(np.uint32), fref.view(np.uint32)
    na, nb = np.isnan(feats), np.isnan(fref)
    print(f"{W}x{H} {mode}: reference NaN words {int(nb.sum())} (negative: {int((nb & (b >> 31 == 1)).sum())}), "
          f"NaN-ness differs in {int((na != nb).sum())} words, non-NaN words differing {int((~na & ~nb & (a != b)).sum())}, "
          f"all words differing {int((a != b).sum())}")
    assert _bits(rgba.cpu().numpy(), cref) == 0
    assert _bits(feats, fref) == 0


# ------------------------------------------------------ 7. mixed and pipelined

def test_features_mixed_and_pipelined(built):
    """render, render_depth and render_features (K = 5) rotating through 8 orbit views, in
    all three phases, on one handle with two frames in flight and depth cuts (feature frames
    invalidate their buffer set's cuts, the colour and depth frames learn them again), into
    reused output tensors: every frame equals a whole-list, one-frame-in-flight handle's."""
    import torch
    W, H, K = 1037, 531, 5
    sc = _scene(100000, 9, 0, W / H, 2.0)
    f = _features(sc.pos.shape[0], K, seed=7)
    views = orbit_views(W, H, 8)
    ref = _hip(sc, depth_split=False, frames_in_flight=1)
    refs = []
    for V, P in views:
        c, d = ref.render_depth_host(V, P, W, H)
        c2, ft = ref.render_features_host(V, P, W, H, f)
        assert _bits(c, c2) == 0
        refs.append((c, d, ft))
    r = _hip(sc, depth_split=True, frames_in_flight=2)
    fd = _dev(f)
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    depth = torch.empty((H, W), dtype=torch.float32, device="cuda:0")
    feats = torch.empty((H, W, K), dtype=torch.float32, device="cuda:0")
    got = []
    for phase in range(3):
        for k, (V, P) in enumerate(views):
            kind = (k + phase) % 3
            if kind == 0:
                r.render(V, P, W, H, out=out)
                got.append((k, out.clone(), None, None))
            elif kind == 1:
                r.render_depth(V, P, W, H, out=out, depth=depth)
                got.append((k, out.clone(), depth.clone(), None))
            else:
                r.render_features(V, P, W, H, fd, out=out, out_features=feats)
                assert r.last_stats()["cut_frame"] == 0
                got.append((k, out.clone(), None, feats.clone()))
    for V, P in views[:3]:  # three consecutive colour frames: depth-cut frames again
        r.render(V, P, W, H, out=out)
    torch.cuda.synchronize()
    assert r.last_stats()["cut_frame"] == 1
    assert _bits(out.cpu().numpy(), refs[2][0]) == 0
    for j, (k, c, d, ft) in enumerate(got):
        rc, rd, rf = refs[k]
        assert _bits(c.cpu().numpy(), rc) == 0, j
        if d is not None:
            assert _bits(d.cpu().numpy(), rd) == 0, j
        if ft is not None:
            assert _bits(ft.cpu().numpy(), rf) == 0, j


# ---------------------------------------------------- 8. after cuts and a jump

@pytest.mark.parametrize("binning", ["bin_first", "depth_first"])
@pytest.mark.parametrize("W,H", [(640, 360), (1037, 531)])
def test_features_after_cuts_and_a_jump(built, W, H, binning):
    """The jump recipe of test_depth_resumed_quadrants (far, far, far, near, near, far, near)
    on a depth-cut handle, with feature frames (K = 4) between its colour frames: colour and
    features equal a whole-list handle's on every frame, and the colour frames still open
    quadrants somewhere in the run.

    A feature frame after every third colour frame, not every second call: these calls are
    host calls, which use one buffer set, and a feature frame invalidates its set's cut
    tables (setup_cuts), so a colour frame that follows a feature frame has whole lists and
    cannot leave a quadrant open.  With every second call a feature frame no colour frame
    would carry cuts at all.  The colour calls follow the recipe's far / near order; the
    feature frame repeats the view of the colour frame before it."""
    from gaussian_splat_amd.api import default_camera
    assert (_bins(W, H) > STRIP_MIN_BINS) == ((W, H) == (1037, 531))
    K = 4
    sc = _scene(400000, 23, 0, W / H, 1.2)
    f = _features(sc.pos.shape[0], K, seed=8)
    cut = _hip(sc, binning=binning, depth_split=True)
    whole = _hip(sc, binning=binning, depth_split=False)
    far = default_camera(W, H)
    far.setDistance(7.0)
    near = default_camera(W, H)
    near.setDistance(2.0)
    near.orbit(0.4, 0.1)
    opened = 0
    for k, cam in enumerate((far, far, far, near, near, far, near)):
        V, P = cam.getViewMatrix(), cam.getProjectionMatrix()
        cb, fb = whole.render_features_host(V, P, W, H, f)
        ca = cut.render_host(V, P, W, H)
        assert _bits(ca, cb) == 0, (k, _bits(ca, cb))
        st = cut.last_stats()
        assert st["cut_frame"] == 1
        opened += st["open_tiles"]
        if k % 3 == 2:
            ca, fa = cut.render_features_host(V, P, W, H, f)
            assert _bits(ca, cb) == 0 and _bits(fa, fb) == 0, (k, _bits(ca, cb), _bits(fa, fb))
            assert cut.last_stats()["cut_frame"] == 0
    print(f"{W}x{H} {binning}: open quadrants (sum) {opened}")
    assert opened > 0


# ------------------------------------------------------------- 9. unsupported

@pytest.mark.parametrize("opts", [dict(cap=32), dict(mode="mlab")])
def test_features_unsupported(built, opts):
    from gaussian_splat_amd._lib import GsError
    W, H = 333, 211
    mode = opts.get("mode", "tile")
    sc = _scene(40000, 7, 0, W / H, 3.0)
    f = _features(sc.pos.shape[0], 4)
    V, P = orbit_views(W, H, 1)[0]
    r = _hip(sc, **opts)
    for call, arg in ((r.render_features, _dev(f)), (r.render_features_host, f)):
        with pytest.raises(GsError) as e:
            call(V, P, W, H, arg)
        assert e.value.status == 7 and "GS_ERR_UNSUPPORTED" in str(e.value), str(e.value)
    from oracle import oracle_py as O
    want, _ = O.render(sc, V, P, W, H, mode=mode, cap=opts.get("cap", 0))
    assert _bits(r.render_host(V, P, W, H), want) == 0


def test_features_sharded_handle_unsupported(built):
    """A handle configured as one rank of two renders its own bin rows only: feature frames
    are whole-frame, so the call is refused before anything is queued."""
    from gaussian_splat_amd._lib import GsError, check, lib
    W, H = 333, 211
    sc = _scene(40000, 7, 0, W / H, 3.0)
    f = _features(sc.pos.shape[0], 4)
    V, P = orbit_views(W, H, 1)[0]
    r = _hip(sc)
    check(lib().gs_shard_configure(r._h, 0, 2, 0), "gs_shard_configure")
    with pytest.raises(GsError) as e:
        r.render_features_host(V, P, W, H, f)
    assert e.value.status == 7 and "gs_render_features" in str(e.value), str(e.value)
    check(lib().gs_shard_configure(r._h, 0, 1, 0), "gs_shard_configure")
    fref = _ref(((40000, 7, 0, W / H, 3.0), W, H, 0), "tile", 4)[4]
    assert _bits(r.render_features_host(V, P, W, H, f)[1], fref) == 0


# -------------------------------------------------------------- 10. host path

def test_features_host_path(built):
    W, H, K = 333, 211, 5
    sc, V, P, f, fref, cref = _ref(((40000, 7, 0, W / H, 3.0), W, H, 0), "tile", K)
    r = _hip(sc)
    fd = _dev(f)
    for k in range(3):
        ch, fh = r.render_features_host(V, P, W, H, f)
        cd, fdev = r.render_features(V, P, W, H, fd)
        assert _bits(ch, cd.cpu().numpy()) == 0 and _bits(fh, fdev.cpu().numpy()) == 0, k
        assert _bits(fh, fref) == 0 and _bits(ch, cref) == 0, k
