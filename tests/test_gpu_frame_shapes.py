"""Every composite path at ragged and extreme frame shapes, against the CPU
oracle bit for bit.

gs_render takes any frame from 1 x 1 to 65535 x 65535.  The shapes here are
the smallest that reach each edge of the two composite kernels (bins are
ceil(W/32) x ceil(H/32); more than 512 bins run composite_strip_kernel, two
pixels per lane at px and px + 8, fewer the one-workgroup-per-tile
composite_kernel):

  strip  1037 x 531   W%32 = 13: the right tile wholly outside, odd width,
                      5 of quadrant B's 8 columns; H%32 = 19: 3 of 16 rows
         1051 x 561   W%32 = 27: 11 of the right tile's 16 columns; one row
         1025 x 545   one pixel column and one pixel row in the last bins
         1040 x 528   the right tile and the bottom half workgroup exactly outside
  tile   333 x 211    the remainders of 1037 x 531
  512 / 513 bins      1024 x 512 (tile), 1025 x 512 (strip)
  4096 px             4096 x 160 (cell masks and 12+4-bit rects), 4097 x 160
                      and 160 x 4097 (plain 16-bit rects)
  16-bit limit        65535 x 32 and 32 x 65535

Every scene carries splats that straddle the right and bottom borders and the
bottom-right corner, and every test first asserts on the oracle's frame that
the last column, the last row and the corner's partial 8 x 8 cell are
covered.  Device outputs lie between guard rows filled with a NaN sentinel:
nothing may be written outside the frame, and every pixel of it must be."""
import functools
import math

import numpy as np
import pytest

from pairs_ref import check_sorted_pairs

pytestmark = pytest.mark.gpu

STRIP_MIN_BINS = 512  # GS_STRIP_MIN_BINS: more bins than this run the strip composite
FULL = [(1037, 531), (1051, 561), (333, 211)]
EXTREME = [(4096, 160), (4097, 160), (160, 4097), (65535, 32), (32, 65535)]
SMALL = [(1025, 545), (1040, 528), (1024, 512), (1025, 512)] + EXTREME
STRIP = {(1037, 531): True, (1051, 561): True, (333, 211): False, (1025, 545): True, (1040, 528): True,
         (1024, 512): False, (1025, 512): True, (4096, 160): True, (4097, 160): True, (160, 4097): True,
         (65535, 32): True, (32, 65535): True, (1037, 1051): True}

SENT_F32 = 0x7FC5A5A5   # a quiet NaN with a payload no arithmetic produces
SENT_BGRA8 = 0x5AC3963C  # (any BGRA8 word can be a live50 pixel: the tests assert the reference has none of these)


def _bins(W, H):
    return ((W + 31) // 32) * ((H + 31) // 32)


def _compare(img, ref):
    diff = np.abs(img.astype(np.float64) - ref.astype(np.float64))
    linf = float(diff.max()) if diff.size else 0.0
    nbit = int(np.count_nonzero(img.view(np.uint32) != ref.view(np.uint32)))
    return linf, nbit


def _camera(W, H, distance=None, orbit=None):
    """The reference's default camera; for frames wider than 4:1 with a
    vertical field of view narrowed until the horizontal one is 79 degrees
    (tan 0.83), so that a 2048:1 frame is still a perspective view."""
    from gaussian_splat_amd.api import default_camera
    cam = default_camera(W, H)
    if W / H > 4.0:
        cam.fov = math.degrees(2.0 * math.atan(math.tan(math.radians(22.5)) * 2.0 * H / W))
    if distance is not None:
        cam.setDistance(distance)
    if orbit is not None:
        cam.orbit(*orbit)
    return cam.getViewMatrix(), cam.getProjectionMatrix()


def _splats_at(V, P, W, H, px, py, rng, sigma_px=2.5, depths=(2.5, 3.0, 3.5, 4.5, 6.0, 8.0)):
    """Splats whose centres project to window positions (px, py), on planes at
    a few view depths (many equal depth keys), about sigma_px pixels wide:
    unprojected through the camera basis (the inverse view matrix)."""
    from gaussian_splat_amd.api import Scene
    n = len(px)
    z = rng.choice(np.asarray(depths), n)
    xv = (2.0 * px / W - 1.0) * z / float(P[0, 0])
    yv = (1.0 - 2.0 * py / H) * z / float(P[1, 1])
    pv = np.stack([xv, yv, -z, np.ones(n)])
    pos = (np.linalg.inv(np.asarray(V, np.float64)) @ pv)[:3].T
    fy = abs(float(P[1, 1])) * H * 0.5  # pixels per unit at view depth 1
    scale = sigma_px * rng.uniform(0.6, 1.6, (n, 3)) * z[:, None] / fy
    return Scene(pos=pos, rot=rng.standard_normal((n, 4)), scale=scale, opacity=rng.uniform(0.2, 0.95, n),
                 color=rng.uniform(0.0, 1.0, (n, 3)))


def _edge_splats(V, P, W, H, rng):
    """Splats straddling the right border, the bottom border and the corner."""
    nr, nb, nc = max(200, H // 6), max(200, W // 6), 24
    px = np.concatenate([rng.uniform(W - 2.5, W + 1.5, nr), rng.uniform(0, W, nb), rng.uniform(W - 1.5, W + 0.5, nc)])
    py = np.concatenate([rng.uniform(0, H, nr), rng.uniform(H - 2.5, H + 1.5, nb), rng.uniform(H - 1.5, H + 0.5, nc)])
    return _splats_at(V, P, W, H, px, py, rng)


def _cat(*scenes):
    from gaussian_splat_amd.api import Scene
    return Scene(*(np.concatenate([getattr(s, f) for s in scenes]) for f in ("pos", "rot", "scale", "opacity", "color")))


@functools.lru_cache(maxsize=None)
def _scene(W, H, n, seed, grow=1.0, frustum=False):
    """(scene, V, P): n splats over the frame plus the border splats of the
    frame's camera.  frustum: the n splats at window positions uniform over
    the whole frame (the extreme shapes, whose ends the synthetic scene's
    crop cube does not reach); otherwise the suite's synthetic scene."""
    from gaussian_splat_amd import scene as S
    V, P = _camera(W, H)
    rng = np.random.default_rng([seed, W, H])
    if frustum:
        body = _splats_at(V, P, W, H, rng.uniform(0, W, n), rng.uniform(0, H, n), rng)
    else:
        body = S.activate(S.synthetic_raw(n, seed=seed, aspect=W / H, rest=False), 0)
        body.scale *= np.float32(grow)
    return _cat(body, _edge_splats(V, P, W, H, rng)), V, P


def _case(W, H, n=40000, seed=7, grow=1.0):
    return _scene(W, H, 30000 if (W, H) in EXTREME else n, seed, grow, (W, H) in EXTREME)


@functools.lru_cache(maxsize=None)
def _oracle(key, mode="tile", cap=0):
    """The oracle's frame of _scene(*key), computed once and left unchanged."""
    from oracle import oracle_py as O
    sc, V, P = _scene(*key)
    ref, _ = O.render(sc, V, P, key[0], key[1], mode=mode, cap=cap)
    ref.setflags(write=False)
    return ref


def _ref(W, H, mode="tile", n=40000, seed=7, grow=1.0, cap=0):
    return _oracle((W, H, 30000 if (W, H) in EXTREME else n, seed, grow, (W, H) in EXTREME), mode, cap)


def _assert_reaches_edges(ref, W, H):
    """Reference-side: the frame's last column, last row and bottom-right
    partial 8 x 8 cell are covered, so the comparison judges them."""
    a = ref[..., 3] > 0
    assert a[:, W - 1].mean() >= 0.25, a[:, W - 1].mean()
    assert a[H - 1, :].mean() >= 0.25, a[H - 1, :].mean()
    assert a[(H - 1) // 8 * 8:, (W - 1) // 8 * 8:].any()


def _assert_path(W, H):
    assert (_bins(W, H) > STRIP_MIN_BINS) == STRIP[(W, H)], (W, H, _bins(W, H))


def _hip(sc, **kw):
    from gaussian_splat_amd import InstancedSplatRenderer, Options
    r = InstancedSplatRenderer(sc, Options(crop=False, **kw))
    r.initialize(0)
    return r


class Guarded:
    """A device frame between two guards of one frame row (rounded up to 4
    words, so the frame stays 16-byte aligned), all filled with a sentinel."""

    def __init__(self, W, H, bgra8=False):
        import torch
        self.W, self.H, self.bgra8 = W, H, bgra8
        wpp = 1 if bgra8 else 4  # 32-bit words per pixel
        self.n = W * H * wpp
        self.g = (W * wpp + 3) // 4 * 4
        self.sent = SENT_BGRA8 if bgra8 else SENT_F32
        self.buf = torch.full((self.n + 2 * self.g,), self.sent, dtype=torch.int32, device="cuda:0")
        mid = self.buf[self.g:self.g + self.n]
        self.out = mid.view(torch.uint8 if bgra8 else torch.float32).view(H, W, 4)
        assert self.out.is_contiguous() and self.out.data_ptr() % 16 == 0

    def frame(self):
        """The frame as a numpy array, after the guard checks."""
        import torch
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy().view(np.uint32)
        g, n = self.g, self.n
        before, after = np.nonzero(raw[:g] != self.sent)[0], np.nonzero(raw[g + n:] != self.sent)[0]
        assert before.size == 0 and after.size == 0, (
            f"{before.size} words written before the frame (first at -{g - int(before[0]) if before.size else 0}), "
            f"{after.size} after it (first at +{int(after[0]) if after.size else 0})")
        mid = raw[g:g + n]
        stale = np.nonzero(mid == self.sent)[0]
        wpp = 1 if self.bgra8 else 4
        assert stale.size == 0, (f"{stale.size} frame words never written, first at pixel "
                                 f"({int(stale[0]) // wpp % self.W}, {int(stale[0]) // wpp // self.W})")
        return mid.view(np.uint8 if self.bgra8 else np.float32).reshape(self.H, self.W, 4).copy()


def _render(r, V, P, W, H):
    g = Guarded(W, H)
    r.render(V, P, W, H, out=g.out)
    return g.frame()


def _render_bgra8(r, V, P, W, H):
    g = Guarded(W, H, bgra8=True)
    r.render_bgra8(V, P, W, H, out=g.out)
    return g.frame()


# ---------------------------------------------------------------- small set

@pytest.mark.parametrize("W,H", SMALL)
def test_default_options(built, W, H):
    """Tile and live50 with default options (the default binning, depth cuts
    on: the second and third frame of a still camera carry cuts)."""
    from oracle import oracle_py as O
    _assert_path(W, H)
    sc, V, P = _case(W, H)
    for mode in ("tile", "live50"):
        ref = _ref(W, H, mode)
        _assert_reaches_edges(ref, W, H)
        r = _hip(sc, mode=mode)
        for k in range(3):
            assert _compare(_render(r, V, P, W, H), ref) == (0.0, 0), (mode, k)
            st = r.last_stats()
            assert st["pairs"] > 0 and st["width"] == W and st["height"] == H
        print(f"{W}x{H} {mode}: pairs {st['pairs']} sorted {st['pairs_sorted']} open {st['open_tiles']}")
    if (W, H) in EXTREME:  # the packed rects reach the last pixel of the long axis
        rec, dk, nt = r.project_host(V, P, W, H)
        orec, odk, ont = O.project(sc, V, P, W, H)
        np.testing.assert_array_equal(nt, ont)
        vis = ont > 0
        np.testing.assert_array_equal(dk[vis], odk[vis])
        np.testing.assert_array_equal(rec[vis].view(np.uint32).reshape(-1, 12), orec[vis].view(np.uint32).reshape(-1, 12))
        x1, y1 = rec["rect_hi"][vis] & 0xFFFF, rec["rect_hi"][vis] >> 16
        assert (x1 == W - 1).any() and (y1 == H - 1).any()
        assert int(x1.max()) == W - 1 and int(y1.max()) == H - 1


# ----------------------------------------------------------------- full set

@pytest.mark.parametrize("W,H", FULL)
def test_rule_and_binning(built, W, H):
    """Both rules, both binning orders with whole lists (equal bin lists), and
    the default options over three frames."""
    _assert_path(W, H)
    sc, V, P = _case(W, H)
    for mode in ("tile", "live50"):
        ref = _ref(W, H, mode)
        _assert_reaches_edges(ref, W, H)
        lists = {}
        for b in ("depth_first", "bin_first"):
            r = _hip(sc, mode=mode, binning=b, depth_split=False)
            assert _compare(_render(r, V, P, W, H), ref) == (0.0, 0), (mode, b)
            lists[b] = r.sorted_pairs() + (r.last_stats()["pairs"],)
        assert lists["depth_first"][2] == lists["bin_first"][2] > 0
        np.testing.assert_array_equal(lists["bin_first"][0], lists["depth_first"][0])
        np.testing.assert_array_equal(lists["bin_first"][1], lists["depth_first"][1])
        r = _hip(sc, mode=mode)
        for k in range(3):
            assert _compare(_render(r, V, P, W, H), ref) == (0.0, 0), (mode, k)
        print(f"{W}x{H} {mode}: pairs {lists['bin_first'][2]}")


@pytest.mark.parametrize("mode,cap", [("tile", 32), ("live50", 50)])
@pytest.mark.parametrize("W,H", FULL)
def test_cap(built, W, H, mode, cap):
    """The per-pixel cap (launch_cap_threshold and the capped composite, both
    on the tile kernel), splats grown x4 so that the cap binds."""
    _assert_path(W, H)
    sc, V, P = _case(W, H, n=20000, seed=21, grow=4.0)
    ref = _ref(W, H, mode, n=20000, seed=21, grow=4.0, cap=cap)
    _assert_reaches_edges(ref, W, H)
    uncapped = _ref(W, H, mode, n=20000, seed=21, grow=4.0)
    assert np.count_nonzero(uncapped.view(np.uint32) != ref.view(np.uint32)) > 0  # the cap changes the frame
    r = _hip(sc, mode=mode, cap=cap)
    assert _compare(_render(r, V, P, W, H), ref) == (0.0, 0)
    assert r.last_stats()["pairs"] > 0
    print(f"{W}x{H} {mode} cap {cap}: pairs {r.last_stats()['pairs']}")
    r.set_cap(0)
    assert _compare(_render(r, V, P, W, H), uncapped) == (0.0, 0)


@pytest.mark.parametrize("W,H", FULL)
def test_mlab(built, W, H):
    _assert_path(W, H)
    sc, V, P = _case(W, H)
    ref = _ref(W, H, "mlab")
    _assert_reaches_edges(ref, W, H)
    r = _hip(sc, mode="mlab")
    assert _compare(_render(r, V, P, W, H), ref) == (0.0, 0)
    assert r.last_stats()["pairs"] > 0
    print(f"{W}x{H} mlab: pairs {r.last_stats()['pairs']}")


@pytest.mark.parametrize("mode", ["tile", "live50"])
@pytest.mark.parametrize("W,H", FULL)
def test_bgra8(built, W, H, mode):
    """BGRA8 output converted inside the composite, whole lists and depth-cut
    frames, into a guarded uint32 frame."""
    _assert_path(W, H)
    from oracle import oracle_py as O
    sc, V, P = _case(W, H)
    ref = _ref(W, H, mode)
    _assert_reaches_edges(ref, W, H)
    want = O.to_bgra8(ref)
    assert not (want.view(np.uint32) == SENT_BGRA8).any()  # (so a frame word with the sentinel was never written)
    for cut in (False, True):
        r = _hip(sc, mode=mode, depth_split=cut)
        for k in range(3 if cut else 1):
            np.testing.assert_array_equal(_render_bgra8(r, V, P, W, H), want)
        assert r.last_stats()["pairs"] > 0
    np.testing.assert_array_equal(r.render_bgra8_host(V, P, W, H), want)


@pytest.mark.parametrize("W,H", FULL)
def test_pair_lists(built, W, H):
    """The bin lists at the ragged shapes, with a few splats blown up x40: no
    duplicates, only bins of the rect, every surely covered bin, the order of
    a stable sort."""
    _assert_path(W, H)
    from oracle import oracle_py as O
    sc, V, P = _case(W, H, n=6001, seed=9)
    sc = _cat(sc)  # (a copy: the cached scene stays as it is)
    idx = np.random.default_rng(W).choice(sc.n, 40, replace=False)
    sc.scale[idx] *= 40.0
    rec, dk, nt = O.project(sc, V, P, W, H)
    for b in ("depth_first", "bin_first"):
        r = _hip(sc, binning=b, depth_split=False)
        _render(r, V, P, W, H)
        keys, vals = r.sorted_pairs()
        npairs, nmust = check_sorted_pairs(keys, vals, rec, dk, nt, W)
        assert npairs == r.last_stats()["pairs"] > 0 and nmust > 0
        assert int(keys.max()) == _bins(W, H) - 1  # the bottom-right bin has a list
    print(f"{W}x{H}: pairs {npairs}")


# --------------------------------------------------------------- depth cuts

CUT_PATH = (7.0, 7.0, 7.0, 2.0, 2.0, 7.0, 2.0)  # far, still; then near and back (camera distances)


@functools.lru_cache(maxsize=None)
def _cut_scene(W, H):
    from gaussian_splat_amd import scene as S
    sc = S.activate(S.synthetic_raw(400000, seed=23, aspect=W / H, rest=False), 0)
    sc.scale *= np.float32(2.0)
    return sc


def _cut_view(W, H, d):
    return _camera(W, H, distance=d, orbit=(0.4, 0.1) if d < 5.0 else None)


@functools.lru_cache(maxsize=None)
def _cut_ref(W, H, mode, d):
    from oracle import oracle_py as O
    ref, _ = O.render(_cut_scene(W, H), *_cut_view(W, H, d), W, H, mode=mode)
    ref.setflags(write=False)
    return ref


def _border(img, W, H):
    """Alpha of the last row, the last column and the corner's partial cell."""
    a = img[..., 3]
    return np.concatenate([a[H - 1, :], a[:, W - 1], a[(H - 1) // 8 * 8:, (W - 1) // 8 * 8:].ravel()])


@pytest.mark.parametrize("mode", ["tile", "live50"])
@pytest.mark.parametrize("binning", ["depth_first", "bin_first"])
@pytest.mark.parametrize("W,H", FULL)
def test_depth_cuts(built, W, H, binning, mode):
    """Depth-cut passes 1 and 2 at the ragged shapes: the far view leaves the
    border quadrants unsaturated and the near view saturates them, so over
    the path they are cut, left open, and resumed from state[pix]."""
    _assert_path(W, H)
    sc = _cut_scene(W, H)
    # both rules stop at T = 0.01: a saturated pixel has alpha >= 1 - 0.01 (fp32)
    sat = np.float32(1.0) - np.float32(0.01)
    far, near = _cut_ref(W, H, mode, 7.0), _cut_ref(W, H, mode, 2.0)
    assert not (_border(far, W, H) >= sat).any()
    assert (_border(near, W, H) >= sat).all()
    cut = _hip(sc, mode=mode, binning=binning, depth_split=True)
    whole = _hip(sc, mode=mode, binning=binning, depth_split=False)
    opened, log = 0, []
    for k, d in enumerate(CUT_PATH):
        V, P = _cut_view(W, H, d)
        a = _render(cut, V, P, W, H)
        assert _compare(a, whole.render_host(V, P, W, H)) == (0.0, 0), k
        st = cut.last_stats()
        assert st["cut_frame"] == 1 and st["pairs"] == whole.last_stats()["pairs"] > 0
        opened += st["open_tiles"]
        log.append((st["pairs"], st["pairs_sorted"], st["open_tiles"]))
        if k == 2:  # the still stretch: the cuts of frame 0 drop pairs
            assert st["pairs_sorted"] < st["pairs"], st
        if k in (0, len(CUT_PATH) - 1):
            assert _compare(a, far if k == 0 else near) == (0.0, 0), k
    assert opened > 0
    print(f"{W}x{H} {mode} {binning}: (pairs, sorted, open tiles) {log} open (sum) {opened}")


# ------------------------------------------------------ two frames in flight

@pytest.mark.parametrize("cut", [False, True])
def test_two_frames_in_flight(built, cut):
    """frames_in_flight 2 over views that alternate the ragged shapes, strip
    and tile kernel: the per-bin buffers (quadrant records, bin order, cuts)
    are re-sized between frames still in flight."""
    from gaussian_splat_amd import scene as S
    from oracle import oracle_py as O
    seq = [(1037, 531), (1051, 561), (1037, 531), (333, 211), (1051, 561), (1051, 561), (333, 211), (1037, 531)]
    rng = np.random.default_rng(33)
    # one scene for the three cameras, with each camera's border splats
    sc = _cat(S.activate(S.synthetic_raw(60000, seed=33, aspect=1037 / 531, rest=False), 0),
              *(_edge_splats(*_camera(W, H), W, H, rng) for W, H in FULL))
    one = _hip(sc, depth_split=False)
    refs = {}
    for W, H in FULL:
        _assert_path(W, H)
        V, P = _camera(W, H)
        refs[(W, H)], _ = O.render(sc, V, P, W, H)
        _assert_reaches_edges(refs[(W, H)], W, H)
        assert _compare(one.render_host(V, P, W, H), refs[(W, H)]) == (0.0, 0), (W, H)  # single-frame renders
    r = _hip(sc, frames_in_flight=2, depth_split=cut)
    outs = []
    for W, H in seq:
        outs.append(Guarded(W, H))
        r.render(*_camera(W, H), W, H, out=outs[-1].out)
    for k, (W, H) in enumerate(seq):
        assert _compare(outs[k].frame(), refs[(W, H)]) == (0.0, 0), k
    assert r.last_stats()["pairs"] > 0


# ------------------------------------------------------------ ranks on 1 GPU

@pytest.mark.parametrize("W,H,worlds,strip", [(1037, 531, (2, 3), False), (1037, 1051, (2,), True)])
def test_ranks_one_gpu(built, W, H, worlds, strip):
    """Row-scheme ranks (virtual shards, the group's rows, pipelined rows) and
    replicated bands on one GPU.  At 1037 x 531 every rank's band stays on the
    tile kernel; at 1037 x 1051 with two ranks each owns 16 or 17 bin rows
    (528 or 561 bins), so its rows / compact band frame runs the strip kernel."""
    from gaussian_splat_amd import ShardedGroup
    from gaussian_splat_amd import distributed as D
    from oracle import oracle_py as O
    sc, V, P = _scene(W, H, 60000, 51)
    V2, P2 = _camera(W, H, orbit=(0.35, 0.1))
    ref = _oracle((W, H, 60000, 51))
    _assert_reaches_edges(ref, W, H)
    ref2, _ = O.render(sc, V2, P2, W, H)
    one = _hip(sc)
    assert _compare(_render(one, V, P, W, H), ref) == (0.0, 0)
    assert one.last_stats()["pairs"] > 0
    _assert_path(W, H)
    for world in worlds:
        owner = D.row_owner(H, world)
        for rank in range(world):
            assert (int((owner == rank).sum()) * ((W + 31) // 32) > STRIP_MIN_BINS) == strip, (world, rank)
        assert _compare(D.render_virtual_shards(sc, world, V, P, W, H), ref) == (0.0, 0), world
        g = ShardedGroup(one, world)
        g.initialize([0] * world, "copy")
        g.set_scheme("rows")
        out = Guarded(W, H)
        g.render(V, P, W, H, out=out.out)
        assert _compare(out.frame(), ref) == (0.0, 0), world
        assert g.last_stats(world - 1)["pairs"] > 0
        g.set_frames_in_flight(2)
        o1, o2 = Guarded(W, H), Guarded(W, H)
        assert g.render_pipelined(V, P, W, H, out=o1.out) is None  # (nothing comes back from the first call)
        assert g.render_pipelined(V2, P2, W, H, out=o1.out) is not None
        assert g.flush(W, H, out=o2.out) is not None
        assert _compare(o1.frame(), ref) == (0.0, 0), world
        assert _compare(o2.frame(), ref2) == (0.0, 0), world
        g.close()
        b = ShardedGroup(one, world, replicated=True)
        b.initialize([0] * world, "copy")
        for (v, p), want in (((V, P), ref), ((V2, P2), ref2)):
            out = Guarded(W, H)
            b.render(v, p, W, H, out=out.out)
            assert _compare(out.frame(), want) == (0.0, 0), world
        b.close()
