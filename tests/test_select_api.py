"""gs_select / gs_prune: the interface, and the host path of handles that were never
initialised, against Scene.subset bit for bit (no GPU compute is called here)."""
import ctypes as C

import numpy as np
import pytest

from select_ref import (GS_ERR_INVALID_ARG, GS_ERR_STATE, GS_OK, payload_scene, prune_masks, scene_diff,
                        select_lists)

N = 1000


def _handle(sh=0, n=N, seed=1):
    from gaussian_splat_amd import InstancedSplatRenderer, Options
    return InstancedSplatRenderer(payload_scene(n, sh, seed), Options(crop=False, sh_degree=sh))  # (not initialised)


def test_library_exports_select_and_prune(built):
    from gaussian_splat_amd import InstancedSplatRenderer, _lib
    for name in ("gs_select", "gs_prune"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().gs_abi_version() == 10  # an addition: the ABI version stays
    assert callable(InstancedSplatRenderer.select) and callable(InstancedSplatRenderer.prune)


def test_bad_arguments_are_rejected(built):
    """Null handle, null index with m > 0, null keep, m = -1 and 2^32 - 1, is_device 2 and -1, a
    host entry equal to n and one of 0xFFFFFFFF: GS_ERR_INVALID_ARG with the call's name in the
    error text on a handle that was never initialised (the arguments are judged first); the
    count and the scene stay as they were.  is_device = 1 on such a handle: GS_ERR_STATE."""
    from gaussian_splat_amd import _lib
    L = _lib.lib()
    r = _handle(sh=1)
    before = r.scene()
    idx = np.arange(N, dtype=np.uint32)
    keep = np.ones(N, np.uint8)
    out = np.full(N, 0x5A5A5A5A, np.uint32)
    cnt = C.c_int64(-7)
    I, K = idx.ctypes.data, keep.ctypes.data

    def unchanged():
        return r.getPointCount() == N and scene_diff(r.scene(), before) == {}

    assert L.gs_select(None, I, N, 0, None) == GS_ERR_INVALID_ARG and "gs_select" in _lib.last_error()
    assert L.gs_prune(None, K, 0, None, None, None) == GS_ERR_INVALID_ARG and "gs_prune" in _lib.last_error()
    for args in ((None, 5, 0), (I, -1, 0), (I, 2 ** 32 - 1, 0), (I, N, 2), (I, N, -1), (None, 5, 1), (I, -1, 1),
                 (I, N, 2 ** 31 - 1)):
        st = L.gs_select(r._h, *args, None)
        assert st == GS_ERR_INVALID_ARG and "gs_select" in _lib.last_error(), (args, st, _lib.last_error())
        assert unchanged(), args
    for args in ((None, 0), (None, 1), (K, 2), (K, -1)):
        st = L.gs_prune(r._h, args[0], args[1], out.ctypes.data, C.byref(cnt), None)
        assert st == GS_ERR_INVALID_ARG and "gs_prune" in _lib.last_error(), (args, st, _lib.last_error())
        assert unchanged(), args
    for bad_value, at in ((N, 0), (N, N - 1), (0xFFFFFFFF, 17), (N + 7, 500)):
        b = idx.copy()
        b[at] = bad_value
        st = L.gs_select(r._h, b.ctypes.data, N, 0, None)
        assert st == GS_ERR_INVALID_ARG and "gs_select" in _lib.last_error(), (bad_value, at, st)
        assert unchanged(), (bad_value, at)
    # a device list / mask on a handle without a device
    assert L.gs_select(r._h, I, N, 1, None) == GS_ERR_STATE and "gs_select" in _lib.last_error()
    assert L.gs_prune(r._h, K, 1, None, None, None) == GS_ERR_STATE and "gs_prune" in _lib.last_error()
    assert unchanged()
    assert (out == 0x5A5A5A5A).all() and cnt.value == -7  # nothing was written by a rejected call
    # and the good calls go through
    assert L.gs_select(r._h, I, N, 0, None) == GS_OK and unchanged()
    assert L.gs_select(r._h, None, 0, 0, None) == GS_OK and r.getPointCount() == 0
    r.close()


@pytest.mark.parametrize("sh", [0, 1, 2, 3])
def test_host_select_equals_subset(built, sh):
    """Every list on a handle that was never initialised: scene() afterwards is subset(index) of
    the scene before, bit for bit in all six arrays (NaN payloads included); two selects compose."""
    for name, idx in select_lists(N).items():
        r = _handle(sh)
        before = r.scene()
        r.select(idx)
        assert r.getPointCount() == idx.size, name
        assert scene_diff(r.scene(), before.subset(idx)) == {}, (sh, name)
        if idx.size:  # a second select on the result: the composition
            again = np.random.default_rng(5).integers(0, idx.size, 2 * idx.size // 3 + 1).astype(np.uint32)
            r.select(again)
            assert scene_diff(r.scene(), before.subset(idx[again])) == {}, (sh, name)
        r.close()
    # other integer dtypes are narrowed after a range check; int32 carries uint32 bits
    r = _handle(sh)
    before = r.scene()
    perm = np.random.default_rng(6).permutation(N)
    r.select(perm.astype(np.int64))
    r.select(np.arange(N, dtype=np.int32)[::-1].copy())
    assert scene_diff(r.scene(), before.subset(perm[::-1])) == {}
    for bad in (np.array([-1], np.int64), np.array([2 ** 32], np.int64)):
        with pytest.raises(ValueError):
            r.select(bad)
    r.close()


@pytest.mark.parametrize("sh", [0, 3])
def test_host_prune_equals_flatnonzero(built, sh):
    """Every mask: the returned map is flatnonzero(keep), its length the new count, scene() the subset."""
    for name, keep in prune_masks(N).items():
        if name == "run":
            continue  # (a device compaction case: no blocks on the host path)
        want = np.flatnonzero(keep)
        for k in (keep, keep.astype(bool)):
            r = _handle(sh)
            before = r.scene()
            got = r.prune(k)
            assert got.dtype == np.uint32 and got.shape == want.shape and (got == want).all(), name
            assert r.getPointCount() == want.size, name
            assert scene_diff(r.scene(), before.subset(want)) == {}, (sh, name)
            r.close()
    assert {int(v) for v in np.unique(prune_masks(N)["values"])} == {0, 1, 255}
    # the C call: out_index past the count is left alone, out_index and out_count may be NULL
    from gaussian_splat_amd import _lib
    L = _lib.lib()
    keep = prune_masks(N)["half"]
    want = np.flatnonzero(keep)
    r = _handle(sh)
    out = np.full(N, 0x5A5A5A5A, np.uint32)
    cnt = C.c_int64(-1)
    assert L.gs_prune(r._h, keep.ctypes.data, 0, out.ctypes.data, C.byref(cnt), None) == GS_OK
    assert cnt.value == want.size and (out[:want.size] == want).all() and (out[want.size:] == 0x5A5A5A5A).all()
    assert L.gs_prune(r._h, np.ones(want.size, np.uint8).ctypes.data, 0, None, None, None) == GS_OK
    assert r.getPointCount() == want.size
    r.close()


def test_shared_planes_keep_their_scene(built):
    """A full-range subset handle shares its source's host planes: one made before a select keeps
    the old scene, one made after sees the new one, and a group created from the handle after a
    select holds the selected scene."""
    from gaussian_splat_amd import _lib
    L = _lib.lib()
    r = _handle(sh=2)
    before = r.scene()
    old = r.subset(0, N)
    idx = select_lists(N)["repeats"]
    r.select(idx)
    assert old.getPointCount() == N and scene_diff(old.scene(), before) == {}
    new = r.subset(0, idx.size)
    part = r.subset(5, 50)
    assert scene_diff(new.scene(), before.subset(idx)) == {}
    assert scene_diff(part.scene(), before.subset(idx[5:50])) == {}
    # ... and the other way round: a select on the sharing handle leaves the source alone
    new.select(np.arange(10, dtype=np.uint32))
    assert r.getPointCount() == idx.size and scene_diff(r.scene(), before.subset(idx)) == {}
    g = C.c_void_p()
    assert L.gs_create_sharded_from_handle(r._h, 2, C.byref(g)) == GS_OK
    assert L.gs_group_point_count(g) == idx.size
    L.gs_group_destroy(g)
    g = C.c_void_p()
    assert L.gs_create_replicated_from_handle(r._h, 2, C.byref(g)) == GS_OK
    assert L.gs_group_point_count(g) == idx.size
    L.gs_group_destroy(g)
    for h in (old, new, part, r):
        h.close()


def test_python_argument_checks(built):
    """A wrong dtype, a wrong length for keep, a non-contiguous argument, a tensor on the CPU and
    anything that is neither a tensor nor an array raise ValueError before the C call: the scene
    is untouched."""
    import torch
    r = _handle()
    before = r.scene()
    for bad in (np.zeros(4, np.float32), np.zeros(4, np.bool_), np.arange(20, dtype=np.uint32)[::2],
                np.zeros((2, 2), np.uint32), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64),
                torch.zeros(4, dtype=torch.float32), [0, 1, 2], None):
        with pytest.raises(ValueError):
            r.select(bad)
    for bad in (np.ones(N, np.int32), np.ones(N, np.float32), np.ones(N - 1, np.uint8), np.ones(N + 1, np.bool_),
                np.ones(2 * N, np.uint8)[::2], np.ones((N, 1), np.uint8), torch.ones(N, dtype=torch.bool),
                torch.ones(N, dtype=torch.uint8), torch.ones(N, dtype=torch.int32), [1] * N, None):
        with pytest.raises(ValueError):
            r.prune(bad)
    assert r.getPointCount() == N and scene_diff(r.scene(), before) == {}
    r.close()
