"""gs_render_depth on the GPU: colour and accumulated depth from one composite pass
(DESIGN.md §2.11), against the CPU oracle bit for bit (tests/depth_ref.py).

Shapes: 333 x 211 runs composite_depth_kernel (77 bins; ragged right and bottom
edges), 1037 x 531 composite_strip_depth_kernel (561 bins; the right tile wholly
outside the frame, 3 of 16 rows in the last bins); 1024 x 512 / 1025 x 512 are the
last tile-kernel and first strip-kernel bin counts (512 / 513)."""
import functools

import numpy as np
import pytest

from conftest import orbit_views
from depth_ref import depth_from_projection, project_zf

pytestmark = pytest.mark.gpu

SENT_F32 = 0x7FC5A5A5  # a quiet NaN with a payload no arithmetic produces
STRIP_MIN_BINS = 512


def _bits(a, b):
    return int(np.count_nonzero(np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)))


def _bins(W, H):
    return ((W + 31) // 32) * ((H + 31) // 32)


def _hip(sc, **kw):
    from gaussian_splat_amd import InstancedSplatRenderer, Options
    r = InstancedSplatRenderer(sc, Options(crop=False, **kw))
    r.initialize(0)
    return r


@functools.lru_cache(maxsize=None)
def _scene(n, seed, sh, aspect, scale):
    from gaussian_splat_amd import scene as S
    sc = S.activate(S.synthetic_raw(n, seed=seed, aspect=aspect, rest=sh > 0), sh)
    sc.scale *= np.float32(scale)
    return sc


@functools.lru_cache(maxsize=None)
def _half_scene(W, H):
    """Splats left of the world's x = -0.5 plane only: the right of the frame stays empty."""
    from gaussian_splat_amd.api import Scene
    sc = _scene(20000, 5, 0, max(W / H, 1.0), 2.0)
    keep = sc.pos[:, 0] < -0.5
    return Scene(pos=sc.pos[keep], rot=sc.rot[keep], scale=sc.scale[keep], opacity=sc.opacity[keep], color=sc.color[keep])


@functools.lru_cache(maxsize=None)
def _projection(key):
    """The oracle's projection with zF of a (scene key, W, H, sh), computed once for both rules."""
    skey, W, H, sh = key
    sc = _half_scene(W, H) if skey == "half" else _scene(*skey)
    V, P = orbit_views(W, H, 1)[0]
    return sc, V, P, project_zf(sc, V, P, W, H, sh)


@functools.lru_cache(maxsize=None)
def _ref(key, mode):
    """(scene, V, P, depth_ref, oracle colour frame), computed once and left unchanged."""
    skey, W, H, sh = key
    sc, V, P, proj = _projection(key)
    depth, colour = depth_from_projection(sc, V, P, W, H, mode, sh, proj)
    return sc, V, P, depth, colour


# ------------------------------------------------------------------ 1. parity

@pytest.mark.parametrize("W,H,mode,cut,sh,scale", [(W, H, m, c, 0, 3.0) for (W, H) in ((333, 211), (1037, 531))
                                                   for m in ("tile", "live50") for c in (False, True)] +
                         [(333, 211, "tile", True, 3, 3.0),
                          # splats x12: lists of many 256-record batches (the software pipeline's
                          # prefetched depths), pixels that saturate (the early outs), lists that are cut
                          (1037, 531, "tile", True, 0, 12.0), (1037, 531, "live50", False, 0, 8.0),
                          (333, 211, "live50", True, 0, 12.0), (333, 211, "tile", False, 0, 12.0)])
def test_depth_parity(built, W, H, mode, cut, sh, scale):
    """Four frames under a still camera (with cuts on, the third and fourth carry
    cuts): depth equals depth_ref on the first and the last frame, colour equals
    gs_render's on a second handle and the oracle's on every frame."""
    assert (_bins(W, H) > STRIP_MIN_BINS) == ((W, H) == (1037, 531))
    sc, V, P, dref, cref = _ref(((40000, 7, sh, W / H, scale), W, H, sh), mode)
    if scale > 3.0:  # both rules stop at T = 0.01: saturated pixels have alpha >= 1 - 0.01 (fp32)
        assert (cref[..., 3] >= np.float32(1.0) - np.float32(0.01)).mean() > 0.25
    assert (cref[..., 3] > 0).mean() > 0.5  # the frame is mostly covered
    r = _hip(sc, mode=mode, depth_split=cut, sh_degree=sh)
    plain = _hip(sc, mode=mode, depth_split=cut, sh_degree=sh)
    for k in range(4):
        rgba, depth = r.render_depth(V, P, W, H)
        rgba, depth = rgba.cpu().numpy(), depth.cpu().numpy()
        st = r.last_stats()
        assert _bits(rgba, plain.render_host(V, P, W, H)) == 0, k
        assert _bits(rgba, cref) == 0, k
        if k in (0, 3):
            assert _bits(depth, dref) == 0, (k, _bits(depth, dref))
        assert st["cut_frame"] == (1 if cut else 0), (k, st)
    print(f"{W}x{H} {mode} cuts {cut} sh {sh} x{scale}: pairs {st['pairs']} sorted {st['pairs_sorted']}")
    # a depth frame's algorithmic composite bytes: 4 B of zF per fetched record and the depth image
    ps = plain.last_stats()
    assert st["records_fetched"] == ps["records_fetched"] > 0
    assert st["bytes_composite"] - ps["bytes_composite"] == 4 * st["records_fetched"] + 4 * W * H


# ------------------------------------------------------------------ 2. bounds

class GuardedDepth:
    """A device depth image between two guards of one frame row (rounded up to 4
    words), all filled with a NaN sentinel."""

    def __init__(self, W, H):
        import torch
        self.W, self.H, self.n, self.g = W, H, W * H, (W + 3) // 4 * 4
        self.buf = torch.full((self.n + 2 * self.g,), SENT_F32, dtype=torch.int32, device="cuda:0")
        self.out = self.buf[self.g:self.g + self.n].view(torch.float32).view(H, W)
        assert self.out.is_contiguous() and self.out.data_ptr() % 16 == 0

    def frame(self):
        import torch
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy().view(np.uint32)
        g, n = self.g, self.n
        assert not (raw[:g] != SENT_F32).any() and not (raw[g + n:] != SENT_F32).any(), "guard words written"
        mid = raw[g:g + n]
        stale = np.nonzero(mid == SENT_F32)[0]
        assert stale.size == 0, (f"{stale.size} depth words never written, first at pixel "
                                 f"({int(stale[0]) % self.W}, {int(stale[0]) // self.W})")
        return mid.view(np.float32).reshape(self.H, self.W).copy()


@pytest.mark.parametrize("W,H", [(1, 1), (17, 9), (1024, 512), (1025, 512)])
def test_depth_bounds(built, W, H):
    """Nothing is written outside the depth image and every pixel of it is, empty
    pixels (and empty bins) with exactly 0.0; then the same shape with the frame
    covered (at 1 x 1 the only pixel is empty in the first scene)."""
    assert (_bins(W, H) > STRIP_MIN_BINS) == ((W, H) == (1025, 512))
    for skey in ("half", (20000, 5, 0, max(W / H, 1.0), 2.0)):
        sc, V, P, dref, cref = _ref((skey, W, H, 0), "tile")
        empty = cref[..., 3] == 0
        if skey == "half":
            assert empty.any() and (dref[empty] == 0.0).all()
        else:
            assert (~empty).any()
        r = _hip(sc)
        for k in range(3):  # (default options: the third frame carries cuts)
            g = GuardedDepth(W, H)
            rgba, _ = r.render_depth(V, P, W, H, depth=g.out)
            depth = g.frame()
            assert _bits(depth, dref) == 0 and _bits(rgba.cpu().numpy(), cref) == 0, (skey, k)
            assert (depth[empty] == 0.0).all()


# ------------------------------------------------------- 3. resumed quadrants

@pytest.mark.parametrize("binning", ["bin_first", "depth_first"])
@pytest.mark.parametrize("W,H", [(640, 360), (1037, 531)])
def test_depth_resumed_quadrants(built, W, H, binning):
    """The jump recipe of test_depth_cuts_jump_opens_tiles: a near view after a
    still stretch leaves quadrants open; pass 1 saves their D beside (C, T) and
    pass 2 resumes it.  Depth and colour equal a whole-list handle's on every frame."""
    from gaussian_splat_amd.api import default_camera
    assert (_bins(W, H) > STRIP_MIN_BINS) == ((W, H) == (1037, 531))
    sc = _scene(400000, 23, 0, W / H, 1.2)
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
        ca, da = cut.render_depth_host(V, P, W, H)
        cb, db = whole.render_depth_host(V, P, W, H)
        assert _bits(ca, cb) == 0 and _bits(da, db) == 0, (k, _bits(ca, cb), _bits(da, db))
        st = cut.last_stats()
        assert st["cut_frame"] == 1
        opened += st["open_tiles"]
    print(f"{W}x{H} {binning}: open quadrants (sum) {opened}")
    assert opened > 0


# ------------------------------------------------------ 4. mixed and pipelined

def test_depth_mixed_and_pipelined(built):
    """render and render_depth alternating on one handle with two frames in flight
    and depth cuts (they share the cut history), into reused output tensors: every
    frame equals a whole-list, one-frame-in-flight handle's."""
    import torch
    W, H = 1037, 531
    sc = _scene(100000, 9, 0, W / H, 2.0)
    views = orbit_views(W, H, 8)
    ref = _hip(sc, depth_split=False, frames_in_flight=1)
    refs = [ref.render_depth_host(V, P, W, H) for V, P in views]
    r = _hip(sc, depth_split=True, frames_in_flight=2)
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    depth = torch.empty((H, W), dtype=torch.float32, device="cuda:0")
    got = []
    for k, (V, P) in enumerate(views):
        if k % 2:
            r.render_depth(V, P, W, H, out=out, depth=depth)
            got.append((out.clone(), depth.clone()))
        else:
            r.render(V, P, W, H, out=out)
            got.append((out.clone(), None))
    # and the other phase: depth frames on the views that were colour frames
    for k, (V, P) in enumerate(views):
        if k % 2:
            r.render(V, P, W, H, out=out)
            got.append((out.clone(), None))
        else:
            r.render_depth(V, P, W, H, out=out, depth=depth)
            got.append((out.clone(), depth.clone()))
    torch.cuda.synchronize()
    assert r.last_stats()["cut_frame"] == 1
    for k, (c, d) in enumerate(got):
        rc, rd = refs[k % len(views)]
        assert _bits(c.cpu().numpy(), rc) == 0, k
        if d is not None:
            assert _bits(d.cpu().numpy(), rd) == 0, k


# ------------------------------------------------------------- 5. unsupported

@pytest.mark.parametrize("opts", [dict(cap=32), dict(mode="mlab")])
def test_depth_unsupported(built, opts):
    from gaussian_splat_amd._lib import GsError
    W, H = 333, 211
    mode = opts.get("mode", "tile")
    sc = _scene(40000, 7, 0, W / H, 3.0)
    V, P = orbit_views(W, H, 1)[0]
    r = _hip(sc, **opts)
    for call in (r.render_depth, r.render_depth_host):
        with pytest.raises(GsError) as e:
            call(V, P, W, H)
        assert e.value.status == 7 and "GS_ERR_UNSUPPORTED" in str(e.value), str(e.value)
    from oracle import oracle_py as O
    want, _ = O.render(sc, V, P, W, H, mode=mode, cap=opts.get("cap", 0))
    assert _bits(r.render_host(V, P, W, H), want) == 0


# --------------------------------------------------------------- 6. host path

def test_depth_host_path(built):
    W, H = 333, 211
    sc, V, P, dref, cref = _ref(((40000, 7, 0, W / H, 3.0), W, H, 0), "tile")
    r = _hip(sc)
    for k in range(3):
        ch, dh = r.render_depth_host(V, P, W, H)
        cd, dd = r.render_depth(V, P, W, H)
        assert _bits(ch, cd.cpu().numpy()) == 0 and _bits(dh, dd.cpu().numpy()) == 0, k
        assert _bits(dh, dref) == 0 and _bits(ch, cref) == 0, k
