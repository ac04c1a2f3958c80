"""Degenerate and non-finite splat values on every path, against the CPU
oracle: 0 pixels whose NaN-ness differs and 0 differing non-NaN bits
(degenerate_zoo.same_frame; a NaN's sign and payload are not part of the
contract).

The scenes are degenerate_zoo's: zero, subnormal, overflowing and NaN
quaternions, scales from 0 to inf, opacities and colours outside [0, 1] and
NaN, non-finite positions and SH coefficients, mixed into the lanes of the
synthetic scene, plus whole waves and a whole workgroup of culled splats.
test_degenerate_oracle.py pins what the oracle makes of each class, so that
these comparisons are not vacuous: full-frame rects, NaN pixels, pixels with
alpha above 1 (negative transmittance) all occur.

Two shapes: 333 x 211 (77 bins, composite_kernel) and 1037 x 531 (561 bins,
composite_strip_kernel).  Device frames lie between guard rows (Guarded of
test_gpu_frame_shapes.py).  NaN frame words are legitimate here, but every
NaN of the scenes is the canonical 0x7FC00000 and arithmetic only produces a
default NaN or hands a payload on, so the guard's payload 0x45A5A5 cannot
occur: each test asserts that on the oracle's frame."""
import functools

import numpy as np
import pytest

from degenerate_zoo import same_frame, same_records, thresholds, zoo
from pairs_ref import check_sorted_pairs
from test_gpu_frame_shapes import SENT_BGRA8, SENT_F32, STRIP_MIN_BINS, Guarded, _bins, _hip, _render, _render_bgra8

pytestmark = pytest.mark.gpu

SHAPES = [(333, 211), (1037, 531)]
STRIP = {(333, 211): False, (1037, 531): True}
SAME = (0, 0)


def _assert_path(W, H):
    assert (_bins(W, H) > STRIP_MIN_BINS) == STRIP[(W, H)], (W, H, _bins(W, H))


def _view(W, H, kind):
    """'still': the zoo's default camera; 'near': a jump towards the scene (as
    test_gpu_depth_split.py's); 'orbit': a second pose for the rank tests."""
    from gaussian_splat_amd.api import default_camera
    cam = default_camera(W, H)
    if kind == "near":
        cam.setDistance(2.0)
        cam.orbit(0.4, 0.1)
    elif kind == "orbit":
        cam.orbit(0.35, 0.1)
    else:
        assert kind == "still"
    return cam.getViewMatrix(), cam.getProjectionMatrix()


@functools.lru_cache(maxsize=None)
def _oracle(W, H, mode="tile", dense=False, cap=0, view="still"):
    """The oracle's frame of zoo(W, H, 0, dense), computed once and left
    unchanged; it never holds the guard sentinel."""
    from oracle import oracle_py as O
    sc = zoo(W, H, 0, dense)[0]
    ref, _ = O.render(sc, *_view(W, H, view), W, H, mode=mode, cap=cap)
    assert not (ref.view(np.uint32) == SENT_F32).any()
    ref.setflags(write=False)
    return ref


def _class_of(classes, i):
    return next((name for name, idx in classes.items() if i in idx), "?")


# ------------------------------------------------------------------ records

@pytest.mark.parametrize("sh", [0, 3])
@pytest.mark.parametrize("W,H", SHAPES)
def test_records(built, W, H, sh):
    """project_host against the oracle's records: the same splats visible,
    equal depth keys, records equal bit for bit (a field that is NaN in the
    oracle's record: NaN)."""
    from oracle import oracle_py as O
    for what in ("zoo", "thresholds"):
        if what == "zoo":
            sc, V, P, classes = zoo(W, H, sh)
        else:
            sc, V, P, d = thresholds(W, H)
            classes = {f"zFront {z:g}": np.array([i]) for i, z in enumerate(d)}
        r = _hip(sc, sh_degree=sh)
        rec, dk, nt = r.project_host(V, P, W, H)
        orec, odk, ont = O.project(sc, V, P, W, H, sh_degree=sh)
        one_side = np.nonzero((nt > 0) != (ont > 0))[0]
        assert one_side.size == 0, [(int(i), _class_of(classes, i), int(nt[i]), int(ont[i])) for i in one_side[:8]]
        bad = np.nonzero(nt != ont)[0]
        assert bad.size == 0, [(int(i), _class_of(classes, i), int(nt[i]), int(ont[i])) for i in bad[:8]]
        vis = ont > 0
        assert vis.any() and not vis.all()
        bad = np.nonzero(vis & (dk != odk))[0]
        assert bad.size == 0, [(int(i), _class_of(classes, i), int(dk[i]), int(odk[i])) for i in bad[:8]]
        if same_records(rec[vis], orec[vis]) != SAME:  # name the first one and its class
            i = next(int(i) for i in np.nonzero(vis)[0] if same_records(rec[i:i + 1], orec[i:i + 1]) != SAME)
            raise AssertionError(f"{what}: record {i} ({_class_of(classes, i)}): {rec[i]} != oracle {orec[i]}")
        print(f"{W}x{H} sh{sh} {what}: {int(vis.sum())} of {sc.n} visible")


# ------------------------------------------------------------------- frames

@pytest.mark.parametrize("mode", ["tile", "live50", "mlab"])
@pytest.mark.parametrize("W,H", SHAPES)
def test_frames(built, W, H, mode):
    """Three frames with default options (the fused projection with the
    scan's reduce half, the default binning, depth cuts from the second frame
    on) into a guarded frame."""
    _assert_path(W, H)
    sc, V, P, _ = zoo(W, H)
    ref = _oracle(W, H, mode)
    assert np.isnan(ref).any()
    r = _hip(sc, mode=mode)
    for k in range(3):
        assert same_frame(_render(r, V, P, W, H), ref) == SAME, (mode, k)
    st = r.last_stats()
    assert st["pairs"] > 0 and st["width"] == W and st["height"] == H
    print(f"{W}x{H} {mode}: pairs {st['pairs']} sorted {st['pairs_sorted']}")


@pytest.mark.parametrize("W,H", SHAPES)
def test_frames_sh3(built, W, H):
    """SH degree 3: NaN, inf and 1e30 coefficients through the colour clamp."""
    from oracle import oracle_py as O
    sc, V, P, _ = zoo(W, H, 3)
    ref, _ = O.render(sc, V, P, W, H, sh_degree=3)
    assert not (ref.view(np.uint32) == SENT_F32).any()
    r = _hip(sc, sh_degree=3)
    for k in range(2):
        assert same_frame(_render(r, V, P, W, H), ref) == SAME, k


@pytest.mark.parametrize("W,H", SHAPES)
def test_thresholds_frame(built, W, H):
    """The splats at the depth thresholds: equal depth keys (the half's
    overflow) composite in index order."""
    from oracle import oracle_py as O
    sc, V, P, _ = thresholds(W, H)
    for mode in ("tile", "mlab"):
        ref, st = O.render(sc, V, P, W, H, mode=mode)
        assert st["visible"] == sc.n - 1 and (ref[..., 3] > 0).any()
        r = _hip(sc, mode=mode)
        assert same_frame(_render(r, V, P, W, H), ref) == SAME, mode


@pytest.mark.parametrize("W,H", SHAPES)
def test_binning(built, W, H):
    """Both binning orders with whole lists: equal bin lists, which pass the
    bin-list rules against the oracle's records (the full-frame classes'
    rects are wider than the 4 x 4 bins a mask can speak for)."""
    from oracle import oracle_py as O
    _assert_path(W, H)
    sc, V, P, _ = zoo(W, H)
    ref = _oracle(W, H)
    orec, odk, ont = O.project(sc, V, P, W, H)
    lists = {}
    for b in ("depth_first", "bin_first"):
        r = _hip(sc, binning=b, depth_split=False)
        assert same_frame(_render(r, V, P, W, H), ref) == SAME, b
        lists[b] = r.sorted_pairs() + (r.last_stats()["pairs"],)
    assert lists["depth_first"][2] == lists["bin_first"][2] > 0
    np.testing.assert_array_equal(lists["bin_first"][0], lists["depth_first"][0])
    np.testing.assert_array_equal(lists["bin_first"][1], lists["depth_first"][1])
    npairs, nmust = check_sorted_pairs(lists["bin_first"][0], lists["bin_first"][1], orec, odk, ont, W)
    assert npairs == lists["bin_first"][2] and nmust > 0
    assert int(lists["bin_first"][0].max()) == _bins(W, H) - 1
    print(f"{W}x{H}: pairs {npairs}, surely covered {nmust}")


@pytest.mark.parametrize("mode,cap", [("tile", 32), ("live50", 50)])
@pytest.mark.parametrize("W,H", SHAPES)
def test_cap(built, W, H, mode, cap):
    """The cap threshold pass and the capped composite on the dense scene,
    where the cap binds."""
    sc, V, P, _ = zoo(W, H, 0, True)
    ref, uncapped = _oracle(W, H, mode, True, cap), _oracle(W, H, mode, True)
    assert same_frame(ref, uncapped) != SAME  # the cap changes the frame
    r = _hip(sc, mode=mode, cap=cap)
    assert same_frame(_render(r, V, P, W, H), ref) == SAME
    assert r.last_stats()["pairs"] > 0
    r.set_cap(0)
    assert same_frame(_render(r, V, P, W, H), uncapped) == SAME


CUT_PATH = ("still", "still", "still", "still", "near", "near", "still", "near")


@pytest.mark.parametrize("mode", ["tile", "live50"])
@pytest.mark.parametrize("binning", ["depth_first", "bin_first"])
@pytest.mark.parametrize("W,H", SHAPES)
def test_depth_cuts(built, W, H, binning, mode):
    """Depth cuts on the dense scene: a still camera for four frames (the
    cuts drop pairs), then jumps towards the scene and back, so that
    quadrants are left open and resumed over bins whose pixels hold NaN and
    negative transmittance (such a pixel never finishes)."""
    _assert_path(W, H)
    sc = zoo(W, H, 0, True)[0]
    cut = _hip(sc, mode=mode, binning=binning, depth_split=True)
    whole = _hip(sc, mode=mode, binning=binning, depth_split=False)
    opened, log = 0, []
    for k, kind in enumerate(CUT_PATH):
        V, P = _view(W, H, kind)
        ref = _oracle(W, H, mode, True, 0, kind)
        a = _render(cut, V, P, W, H)
        assert same_frame(a, whole.render_host(V, P, W, H)) == SAME, k
        assert same_frame(a, ref) == SAME, k
        st = cut.last_stats()
        assert st["cut_frame"] == 1 and st["pairs"] == whole.last_stats()["pairs"] > 0
        opened += st["open_tiles"]
        log.append((st["pairs"], st["pairs_sorted"], st["open_tiles"]))
        if k == 3:
            assert st["pairs_sorted"] < st["pairs"], st
    assert opened > 0
    print(f"{W}x{H} {mode} {binning}: (pairs, sorted, open tiles) {log}")


@pytest.mark.parametrize("mode", ["tile", "live50"])
def test_bgra8(built, mode):
    """BGRA8 of NaN, negative and above-1 channels, converted inside the
    composite and on the host, whole lists and depth-cut frames."""
    from oracle import oracle_py as O
    W, H = 1037, 531
    _assert_path(W, H)
    sc, V, P, _ = zoo(W, H)
    ref = _oracle(W, H, mode)
    assert np.isnan(ref).any() and (ref > 1).any()
    if mode == "tile":  # (the live-50 rule's colours only grow)
        assert (ref[..., :3] < 0).any()
    want = O.to_bgra8(ref)
    assert not (want.view(np.uint32) == SENT_BGRA8).any()
    for cut in (False, True):
        r = _hip(sc, mode=mode, depth_split=cut)
        for k in range(3 if cut else 1):
            assert same_frame(_render_bgra8(r, V, P, W, H), want) == SAME, (cut, k)
    assert same_frame(r.render_bgra8_host(V, P, W, H), want) == SAME


# ------------------------------------------------------------ ranks on 1 GPU

@pytest.mark.parametrize("world", [2, 3])
def test_ranks_one_gpu(built, world):
    """Row-scheme virtual shards (the projection's destination counts) and
    replicated bands (the band cull before the covariance, with NaN and inf
    splats) on one GPU, against the single-GPU frame and the oracle."""
    from gaussian_splat_amd import ShardedGroup
    from gaussian_splat_amd import distributed as D
    W, H = 1037, 531
    sc = zoo(W, H)[0]
    views = [(_view(W, H, kind), _oracle(W, H, "tile", False, 0, kind)) for kind in ("still", "orbit")]
    one = _hip(sc)
    single = [_render(one, V, P, W, H) for (V, P), _ in views]
    for img, (_, ref) in zip(single, views):
        assert same_frame(img, ref) == SAME
    (V, P), ref = views[0]
    shards = D.render_virtual_shards(sc, world, V, P, W, H)
    assert same_frame(shards, ref) == SAME and same_frame(shards, single[0]) == SAME
    b = ShardedGroup(one, world, replicated=True)
    b.initialize([0] * world, "copy")
    for img, ((v, p), want) in zip(single, views):
        out = Guarded(W, H)
        b.render(v, p, W, H, out=out.out)
        band = out.frame()
        assert same_frame(band, want) == SAME and same_frame(band, img) == SAME
    assert b.last_stats(world - 1)["pairs"] > 0
    b.close()


# ------------------------------------------------------ two frames in flight

@pytest.mark.parametrize("cut", [False, True])
def test_two_frames_in_flight(built, cut):
    """frames_in_flight 2 over views that alternate the two shapes (strip and
    tile kernel) of one zoo scene."""
    from oracle import oracle_py as O
    seq = [(1037, 531), (333, 211), (1037, 531), (1037, 531), (333, 211), (333, 211), (1037, 531)]
    sc = zoo(1037, 531)[0]
    refs = {}
    for W, H in SHAPES:
        _assert_path(W, H)
        refs[(W, H)], _ = O.render(sc, *_view(W, H, "still"), W, H)
        assert np.isnan(refs[(W, H)]).any() and not (refs[(W, H)].view(np.uint32) == SENT_F32).any()
    r = _hip(sc, frames_in_flight=2, depth_split=cut)
    outs = []
    for W, H in seq:
        outs.append(Guarded(W, H))
        r.render(*_view(W, H, "still"), W, H, out=outs[-1].out)
    for k, (W, H) in enumerate(seq):
        assert same_frame(outs[k].frame(), refs[(W, H)]) == SAME, k
    assert r.last_stats()["pairs"] > 0
