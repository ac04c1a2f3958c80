"""gs_select / gs_prune on the GPU: the handle's planes re-indexed on the device (select.hip,
DESIGN.md §7).  After either call the handle is indistinguishable from a fresh one created with
the same options from scene().subset(index): same scene bits, same frames (0 differing bits),
on every render call.

B = 1024 is the compaction kernel's block (kSelectBlock: four waves of 256 mask bytes); the
gather runs 256 splats per block.  Fresh handles are built with crop=False from the subset of
the scene the handle held before the call."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import orbit_views
from depth_ref import project_zf
from select_ref import (GS_ERR_INVALID_ARG, GS_ERR_UNSUPPORTED, GS_OK, SELECT_BLOCK, payload_scene, prune_masks,
                        scene_diff, select_lists)
from test_gpu_depth_output import _bits, _hip, _scene

pytestmark = pytest.mark.gpu

B = SELECT_BLOCK
SIZES = [1, 63, 64, 65, B - 1, B, B + 1, 3 * B + 1]


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def _dev_index(idx):
    """A uint32 list as the torch.int32 tensor holding its bits (render_ids' convention)."""
    return _dev(np.ascontiguousarray(idx, np.uint32).view(np.int32))


def _frame(r, V, P, W, H):
    return r.render(V, P, W, H).cpu().numpy()


# ------------------------------------------------------------------ 1. planes, small sizes

@functools.lru_cache(maxsize=None)
def _small(n, sh):
    sc = payload_scene(n, sh, seed=3)
    sc.scale *= np.float32(8.0)  # (a 64 x 48 frame: splats a few pixels wide)
    return sc


@pytest.mark.parametrize("sh", [0, 1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_planes_small_sizes(built, n, sh):
    """Every mask and every list at the sizes around the wave, the compaction block and several
    blocks: the device map is flatnonzero(keep), the count is right, scene() is the subset and a
    64 x 48 frame is a fresh handle's; the device path and the host path of an initialised handle
    agree."""
    import torch
    W, H = 64, 48
    V, P = orbit_views(W, H, 1)[0]
    sc = _small(n, sh)
    opt = dict(sh_degree=sh)
    masks = prune_masks(n)
    if n > B:
        run = np.flatnonzero(masks["run"])
        assert run[0] < B <= run[-1] and run.size == run[-1] - run[0] + 1  # one run over a block boundary
    for name, keep in masks.items():
        want = np.flatnonzero(keep)
        r = _hip(sc, **opt)
        before = r.scene()
        got = r.prune(_dev(keep) if name != "half" else _dev(keep.astype(bool)))
        assert got.is_cuda and got.dtype == torch.int32
        got = got.cpu().numpy().view(np.uint32)
        assert got.shape == want.shape and (got == want).all(), (name, got[:8], want[:8])
        assert r.getPointCount() == want.size, name
        assert scene_diff(r.scene(), before.subset(want)) == {}, name
        fresh = _hip(before.subset(want), **opt)
        assert _bits(_frame(r, V, P, W, H), _frame(fresh, V, P, W, H)) == 0, name
        # the host mask on an initialised handle: the same compaction, the same result
        rh = _hip(sc, **opt)
        gh = rh.prune(keep)
        assert gh.dtype == np.uint32 and (gh == want).all() and scene_diff(rh.scene(), r.scene()) == {}, name
        assert _bits(rh.render_host(V, P, W, H), _frame(fresh, V, P, W, H)) == 0, name
        for h in (r, rh, fresh):
            h.close()
    lists = select_lists(n)
    for name in ("reversal", "permutation", "repeats", "none"):
        idx = lists[name]
        rd, rh = _hip(sc, **opt), _hip(sc, **opt)
        before = rd.scene()
        rd.select(_dev_index(idx) if name != "permutation" else _dev(idx.astype(np.int64)))
        rh.select(idx)
        assert rd.getPointCount() == rh.getPointCount() == idx.size, name
        assert scene_diff(rd.scene(), before.subset(idx)) == {}, name
        assert scene_diff(rh.scene(), before.subset(idx)) == {}, name
        fresh = _hip(before.subset(idx), **opt)
        f = _frame(fresh, V, P, W, H)
        assert _bits(_frame(rd, V, P, W, H), f) == 0 and _bits(rh.render_host(V, P, W, H), f) == 0, name
        if name == "repeats":
            assert idx.size > n
        for h in (rd, rh, fresh):
            h.close()


# ------------------------------------------------------------------ 2. frames against the oracle

@functools.lru_cache(maxsize=None)
def _oracle_half(sh, mode):
    """(scene, keep, V, P, oracle frame of the whole scene, oracle frame of the kept half)."""
    from oracle import oracle_py as O
    W, H = 333, 211
    sc = _scene(40000, 7, sh, W / H, 3.0)
    V, P = orbit_views(W, H, 1)[0]
    keep = (np.random.default_rng(41).random(sc.n) < 0.5).astype(np.uint8)
    whole, _ = O.render(sc, V, P, W, H, sh_degree=sh, mode=mode)
    half, _ = O.render(sc.subset(np.flatnonzero(keep)), V, P, W, H, sh_degree=sh, mode=mode)
    return sc, keep, V, P, whole, half


@pytest.mark.parametrize("mode", ["tile", "live50"])
@pytest.mark.parametrize("sh", [0, 3])
def test_pruned_frames_equal_the_oracle(built, sh, mode):
    """40 000 splats at 333 x 211, a seeded half kept on the device: the colour frame is the CPU
    oracle's frame of the subset scene and a fresh handle's; the prune changes more than a tenth
    of the pixels (checked on the oracle alone)."""
    W, H = 333, 211
    sc, keep, V, P, whole, half = _oracle_half(sh, mode)
    changed = (whole.view(np.uint32) != half.view(np.uint32)).any(axis=-1).mean()
    assert changed > 0.10, changed
    r = _hip(sc, mode=mode, sh_degree=sh)
    before = r.scene()
    assert _bits(_frame(r, V, P, W, H), whole) == 0
    idx = r.prune(_dev(keep)).cpu().numpy().view(np.uint32)
    assert (idx == np.flatnonzero(keep)).all()
    fresh = _hip(before.subset(idx), mode=mode, sh_degree=sh)
    for k in range(3):  # (with depth cuts on: the third frame carries cuts learnt on the pruned scene)
        f = _frame(r, V, P, W, H)
        assert _bits(f, half) == 0, (k, _bits(f, half))
        assert _bits(f, _frame(fresh, V, P, W, H)) == 0, k


# ------------------------------------------------------------------ 3. history does not leak

@functools.lru_cache(maxsize=None)
def _depth_halves():
    """100 000 splats at 1037 x 531 and the oracle's zF of the still view: masks keeping the far
    and the near half of the splats ahead of the camera."""
    W, H = 1037, 531
    sc = _scene(100000, 9, 0, W / H, 3.0)
    V, P = orbit_views(W, H, 1)[0]
    rec, dkey, ntiles, zf = project_zf(sc, V, P, W, H, 0)
    mid = np.median(zf[ntiles > 0])
    far = (zf > mid).astype(np.uint8)  # near half pruned away
    near = (zf <= mid).astype(np.uint8)
    assert 0.3 < far.mean() < 0.7 and 0.3 < near.mean() < 0.7
    return sc, V, P, {"near_removed": far, "far_removed": near}


@pytest.mark.parametrize("binning", ["default", "depth_first", "bin_first"])
@pytest.mark.parametrize("which", ["near_removed", "far_removed"])
def test_history_does_not_leak(built, which, binning):
    """Strip-kernel frames with depth cuts and two frames in flight under a still camera: four
    frames learn cuts, then the near (or far) half goes and four more frames each equal a
    whole-list fresh handle's on the pruned scene; with the near half gone the tiles saturate
    deeper than the cuts they had learnt.  Cuts are in use again by the last frame."""
    W, H = 1037, 531
    sc, V, P, halves = _depth_halves()
    keep = halves[which]
    r = _hip(sc, depth_split=True, frames_in_flight=2, binning=binning)
    first = [_frame(r, V, P, W, H) for _ in range(4)]
    st = r.last_stats()
    assert st["cut_frame"] == 1, st  # depth-cut frames: cuts learnt
    assert all(_bits(f, first[0]) == 0 for f in first)
    before = r.scene()
    idx = r.prune(_dev(keep)).cpu().numpy().view(np.uint32)
    fresh = _hip(before.subset(idx), depth_split=False, frames_in_flight=1, binning=binning)
    want = _frame(fresh, V, P, W, H)
    assert _bits(want, first[0]) > 0
    for k in range(4):
        f = _frame(r, V, P, W, H)
        assert _bits(f, want) == 0, (which, binning, k, _bits(f, want))
        st = r.last_stats()
        assert st["splats"] == idx.size and st["cut_frame"] == 1, (k, st)
        if k == 0:  # no cut of the old scene survives: the first frame's lists are whole
            assert st["pairs_sorted"] == st["pairs"] and st["cut_dilate"] == 0, st
    assert st["cut_frame"] == 1 and st["pairs_sorted"] <= st["pairs"], st


# ------------------------------------------------------------------ 4. all render calls after a permutation

def test_every_render_call_after_a_reversal(built):
    """The reversed scene (every depth tie's arrival order flips) at 333 x 211: depth, features
    (rows re-indexed with the same list), contrib, ids and bgra8 frames equal a fresh handle's,
    as do a cap = 32 tile frame and an MLAB frame; ids name the same old splats as before the
    reversal wherever a pixel's candidates all fit the slots with distinct, unchanged q."""
    import torch
    W, H = 333, 211
    sc = _scene(40000, 7, 0, W / H, 3.0)
    V, P = orbit_views(W, H, 2)[1]
    orig = _hip(sc)
    r = _hip(sc)
    before = r.scene()
    rev = np.arange(sc.n, dtype=np.uint32)[::-1].copy()
    r.select(_dev_index(rev))
    fresh = _hip(before.subset(rev))
    assert scene_diff(r.scene(), fresh.scene()) == {}
    eq = lambda a, b: bool(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                       b.view(torch.int32) if b.dtype == torch.float32 else b))
    for a, b in zip(r.render_depth(V, P, W, H), fresh.render_depth(V, P, W, H)):
        assert eq(a, b)
    feats = np.random.default_rng(8).standard_normal((sc.n, 4)).astype(np.float32)
    fa = r.render_features(V, P, W, H, _dev(feats[rev]))
    fb = fresh.render_features(V, P, W, H, _dev(feats[rev]))
    fo = orig.render_features(V, P, W, H, _dev(feats))
    assert eq(fa[0], fb[0]) and eq(fa[1], fb[1])
    assert (fa[1] != 0).any() and fo[1].shape == fa[1].shape
    ca, cb = r.render_contrib(V, P, W, H), fresh.render_contrib(V, P, W, H)
    assert all(eq(a, b) for a, b in zip(ca, cb)) and int(ca[2].sum()) > 0
    ia, ib = r.render_ids(V, P, W, H, slots=4), fresh.render_ids(V, P, W, H, slots=4)
    assert all(eq(a, b) for a, b in zip(ia, ib))
    assert eq(r.render_bgra8(V, P, W, H), fresh.render_bgra8(V, P, W, H))
    # ids, mapped through the list, against the handle that still holds the old order
    io = orig.render_ids(V, P, W, H, slots=4)
    ids_n, q_n, cnt_n = (t.cpu().numpy().view(np.uint32) for t in ia[1:])
    ids_o, q_o, cnt_o = (t.cpu().numpy().view(np.uint32) for t in io[1:])
    filled = np.arange(4)[None, None, :] < np.minimum(cnt_n, 4)[..., None]
    distinct = ((q_n[..., :-1] != q_n[..., 1:]) | ~filled[..., 1:]).all(axis=-1)
    ok = distinct & (cnt_n <= 4) & (cnt_n == cnt_o) & (q_n == q_o).all(axis=-1) & (cnt_n > 0)
    assert ok.sum() > 0
    print(f"ids after a reversal: {ok.mean():.3f} of the pixels compared")
    mapped = np.where(filled, rev[np.minimum(ids_n, sc.n - 1)], np.uint32(0xFFFFFFFF))
    assert (mapped[ok] == ids_o[ok]).all()
    for h in (r, fresh):
        h.set_cap(32)
    assert eq(r.render(V, P, W, H), fresh.render(V, P, W, H))
    for h in (r, fresh):
        h.set_cap(0)
        h.set_mode("mlab")
    assert eq(r.render(V, P, W, H), fresh.render(V, P, W, H))


# ------------------------------------------------------------------ 5. the loop the feature exists for

def test_prune_by_contrib_over_three_views(built):
    """render_contrib over three orbit views accumulating, keep = sum > 0 on the device, prune:
    the count drops, the three views equal the oracle's frames of the subset scene and a fresh
    handle's, and equal the frames before the prune wherever the oracle says they do."""
    import torch
    from contrib_ref import contrib_ref
    from oracle import oracle_py as O
    W, H = 160, 96
    sc = _scene(2000, 7, 0, W / H, 20.0)  # (splats large enough to hide a few others from all three views)
    views = orbit_views(W, H, 3)
    total = np.zeros(sc.n, np.uint64)
    for V, P in views:
        total += contrib_ref(sc, V, P, W, H, "tile")[0]
    want_keep = total > 0
    assert 0 < int(want_keep.sum()) < sc.n  # at least one splat goes and one stays
    r = _hip(sc)
    before = r.scene()
    s = torch.zeros(sc.n, dtype=torch.int64, device="cuda:0")
    c = torch.zeros(sc.n, dtype=torch.int32, device="cuda:0")
    m = torch.zeros(sc.n, dtype=torch.int32, device="cuda:0")
    pre = []
    for V, P in views:
        pre.append(r.render_contrib(V, P, W, H, sum=s, count=c, max=m, accumulate=True)[0].cpu().numpy())
    keep = s > 0
    assert (keep.cpu().numpy() == want_keep).all()
    idx = r.prune(keep).cpu().numpy().view(np.uint32)
    assert (idx == np.flatnonzero(want_keep)).all() and r.getPointCount() == idx.size < sc.n
    sub = before.subset(idx)
    fresh = _hip(sub)
    differing = 0
    for k, (V, P) in enumerate(views):
        f = _frame(r, V, P, W, H)
        assert _bits(f, _frame(fresh, V, P, W, H)) == 0, k
        o_sub, _ = O.render(sub, V, P, W, H, mode="tile")
        o_all, _ = O.render(sc, V, P, W, H, mode="tile")
        assert _bits(f, o_sub) == 0, k
        # (a dropped splat has q = 0 at every pixel but may carry weight below 2^-24)
        px = int((o_sub.view(np.uint32) != o_all.view(np.uint32)).any(axis=-1).sum())
        got = int((f.view(np.uint32) != pre[k].view(np.uint32)).any(axis=-1).sum())
        assert got == px, (k, got, px)
        differing += px
    print(f"prune by contrib: {sc.n} -> {idx.size} splats, {differing} pixels differ from the frames before")


# ------------------------------------------------------------------ 6. rejected device list

def test_rejected_device_list_leaves_the_handle_alone(built):
    """n = 1000: a device list with one entry equal to n, another with n + 7 (inside the slack of
    the plane allocations): GS_ERR_INVALID_ARG, the count and the next frame as before.  A handle
    configured as one rank of two: GS_ERR_UNSUPPORTED."""
    from gaussian_splat_amd import _lib
    L = _lib.lib()
    W, H = 64, 48
    V, P = orbit_views(W, H, 1)[0]
    n = 1000
    sc = _small(n, 3)
    r = _hip(sc, sh_degree=3)
    want = _frame(r, V, P, W, H)
    before = r.scene()
    for bad, at in ((n, 0), (n + 7, 613), (n, n - 1)):
        idx = np.random.default_rng(at).permutation(n).astype(np.uint32)
        idx[at] = bad
        t = _dev_index(idx)
        st = L.gs_select(r._h, C.c_void_p(t.data_ptr()), n, 1, None)
        assert st == GS_ERR_INVALID_ARG and "gs_select" in _lib.last_error(), (bad, at, st, _lib.last_error())
        assert r.getPointCount() == n and scene_diff(r.scene(), before) == {}
        assert _bits(_frame(r, V, P, W, H), want) == 0, (bad, at)
    with pytest.raises(_lib.GsError):
        r.select(_dev_index(np.array([3, n, 5], np.uint32)))
    assert r.getPointCount() == n and _bits(_frame(r, V, P, W, H), want) == 0
    assert L.gs_shard_configure(r._h, 0, 2, 0) == GS_OK
    keep, ident = _dev(np.ones(n, np.uint8)), _dev_index(np.arange(n))
    assert L.gs_select(r._h, C.c_void_p(ident.data_ptr()), n, 1, None) == GS_ERR_UNSUPPORTED
    assert "gs_select" in _lib.last_error()
    assert L.gs_prune(r._h, C.c_void_p(keep.data_ptr()), 1, None, None, None) == GS_ERR_UNSUPPORTED
    assert "gs_prune" in _lib.last_error()
    assert r.getPointCount() == n and scene_diff(r.scene(), before) == {}


# ------------------------------------------------------------------ 7. reuse

def test_ten_prunes_on_one_handle(built):
    """Ten seeded 80 % prunes alternating with frames on one handle (two frames in flight, depth
    cuts): every frame equals a fresh handle's, the last scene the composed subset."""
    W, H = 333, 211
    sc = _scene(40000, 7, 0, W / H, 3.0)
    V, P = orbit_views(W, H, 1)[0]
    r = _hip(sc, frames_in_flight=2, depth_split=True)
    start = r.scene()
    composed = np.arange(sc.n)
    rng = np.random.default_rng(77)
    for k in range(10):
        _frame(r, V, P, W, H)
        keep = (rng.random(r.getPointCount()) < 0.8).astype(np.uint8)
        idx = r.prune(_dev(keep)).cpu().numpy().view(np.uint32)
        composed = composed[idx]
        assert r.getPointCount() == composed.size
        fresh = _hip(start.subset(composed), frames_in_flight=1, depth_split=False)
        a, b = _frame(r, V, P, W, H), _frame(fresh, V, P, W, H)
        assert _bits(a, b) == 0, (k, _bits(a, b))
        fresh.close()
    assert composed.size < 0.2 * sc.n
    assert scene_diff(r.scene(), start.subset(composed)) == {}
