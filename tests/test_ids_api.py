"""gs_render_ids' interface and its CPU reference (no GPU compute is called here)."""
import ctypes as C

import numpy as np
import pytest

from conftest import orbit_views
from contrib_ref import contrib_fragments
from depth_ref import project_zf
from ids_ref import ID_NONE, ids_loop, ids_ref, tie_counts

GS_ERR_INVALID_ARG = 1
SENT32 = 0x5A5A5A5A


def test_library_exports_gs_render_ids(built):
    from gaussian_splat_amd import _lib
    assert "gs_render_ids" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "gs_render_ids")
    assert _lib.lib().gs_abi_version() == 10  # an addition: the ABI version stays


def test_bad_arguments_are_rejected(built):
    """Null handle, view, proj, out_rgba or out_ids, a size outside 1..65535, slots outside
    1..4, is_device outside {0, 1}: GS_ERR_INVALID_ARG with the call's name in the error text,
    also on a handle that was never initialised (the arguments are judged first), and the
    outputs stay untouched.  Good arguments, NULL out_q and NULL out_count among them, get
    past the check to the handle's state."""
    from gaussian_splat_amd import InstancedSplatRenderer, Options, _lib
    from gaussian_splat_amd import scene as S
    L = _lib.lib()
    m = np.eye(4, dtype=np.float32).reshape(16)
    fp = m.ctypes.data_as(C.POINTER(C.c_float))
    nofp = C.POINTER(C.c_float)()
    rgba = np.zeros(4 * 4 * 4, np.float32)
    ids, q, cnt = (np.full(n, SENT32, np.uint32) for n in (64, 64, 16))
    R, I, Q, N = rgba.ctypes.data, ids.ctypes.data, q.ctypes.data, cnt.ctypes.data
    assert L.gs_render_ids(None, fp, fp, 4, 4, 4, R, I, Q, N, 0, None) == GS_ERR_INVALID_ARG
    assert "gs_render_ids" in _lib.last_error()
    r = InstancedSplatRenderer(S.synthetic_scene(100, seed=1), Options(crop=False))  # (created, not initialised)
    good = dict(view=fp, proj=fp, w=4, h=4, slots=4, rgba=R, ids=I, q=Q, cnt=N, dev=0)

    def call(a):
        return L.gs_render_ids(r._h, a["view"], a["proj"], a["w"], a["h"], a["slots"], a["rgba"], a["ids"], a["q"],
                               a["cnt"], a["dev"], None)

    bad = [dict(view=nofp), dict(proj=nofp), dict(rgba=None), dict(ids=None),
           dict(w=0), dict(h=0), dict(w=-3), dict(h=-1), dict(w=65536), dict(h=65536),
           dict(slots=0), dict(slots=-1), dict(slots=5), dict(dev=2), dict(dev=-1)]
    for case in bad:
        st = call({**good, **case})
        assert st == GS_ERR_INVALID_ARG, (case, st)
        assert "gs_render_ids" in _lib.last_error(), (case, _lib.last_error())
    # good arguments pass the argument check: the handle's state is judged next
    for case in (dict(), dict(q=None), dict(cnt=None), dict(q=None, cnt=None), dict(slots=1), dict(slots=2),
                 dict(slots=3), dict(dev=1), dict(w=65535, h=1), dict(w=1, h=65535)):
        st = call({**good, **case})
        assert st != GS_ERR_INVALID_ARG and "gs_initialize" in _lib.last_error(), (case, st, _lib.last_error())
    assert (ids == SENT32).all() and (q == SENT32).all() and (cnt == SENT32).all() and not rgba.any()
    r.close()


def test_python_interface_has_render_ids(built):
    """The methods exist; slots outside 1..4, a CPU tensor, a wrong dtype, a wrong size and a
    non-contiguous tensor raise ValueError before the C call."""
    import torch
    from gaussian_splat_amd import InstancedSplatRenderer, Options
    from gaussian_splat_amd import scene as S
    assert callable(InstancedSplatRenderer.render_ids) and callable(InstancedSplatRenderer.render_ids_host)
    r = InstancedSplatRenderer(S.synthetic_scene(100, seed=1), Options(crop=False))  # (created, not initialised)
    W, H = 16, 8
    V, P = orbit_views(W, H, 1)[0]
    for kw in (dict(slots=0), dict(slots=5), dict(slots=-1),
               dict(ids=torch.zeros((H, W, 4), dtype=torch.int32)),  # on the CPU
               dict(q=torch.zeros((H, W, 4), dtype=torch.int32)), dict(count=torch.zeros((H, W), dtype=torch.int32)),
               dict(ids=torch.zeros((H, W, 4), dtype=torch.int64)), dict(ids=torch.zeros((H, W, 3), dtype=torch.int32)),
               dict(count=torch.zeros((H, 2 * W), dtype=torch.int32)[:, ::2]), dict(ids=np.zeros((H, W, 4), np.uint32))):
        with pytest.raises(ValueError):
            r.render_ids(V, P, W, H, **kw)
    for kw in (dict(slots=0), dict(slots=5)):
        with pytest.raises(ValueError):
            r.render_ids_host(V, P, W, H, **kw)
    r.close()


@pytest.fixture(scope="module")
def tiny_frame():
    from test_gpu_frame_shapes import _splats_at
    W, H = 17, 9
    V, P = orbit_views(W, H, 1)[0]
    rng = np.random.default_rng(3)  # (120 splats about 3 px wide over the whole frame: many per pixel)
    sc = _splats_at(V, P, W, H, rng.uniform(0, W, 120), rng.uniform(0, H, 120), rng, sigma_px=3.0)
    return sc, V, P, W, H, project_zf(sc, V, P, W, H)


@pytest.mark.parametrize("mode", ["tile", "live50"])
def test_reference_agrees_with_a_plain_loop(built, tiny_frame, mode):
    """ids_ref against a per-pixel Python loop over the oracle's fragments of a 17 x 9 frame,
    both rules, K = 1..4; the frame has pixels with more than four candidates (eviction) and
    the properties every result has."""
    sc, V, P, W, H, proj = tiny_frame
    fr = contrib_fragments(sc, V, P, W, H, mode, 0, proj)
    assert fr[0].size > W * H
    for K in (1, 2, 3, 4):
        got, want = ids_ref(fr, W, H, K), ids_loop(fr, W, H, K)
        for name, g, w in zip(("ids", "q", "count"), got, want):
            assert g.dtype == np.uint32 and g.shape == w.shape and (g == w).all(), (K, name)
        ids, q, count = got
        assert ids.shape == (H, W, K) and q.shape == (H, W, K) and count.shape == (H, W)
        assert (count > 4).any()
        filled = np.arange(K)[None, None, :] < np.minimum(count, K)[..., None]
        assert ((ids != ID_NONE) == filled).all() and ((q > 0) == filled).all()
        assert (q[..., :-1] >= q[..., 1:]).all() and (q <= (1 << 24)).all()
        tie = (q[..., :-1] == q[..., 1:]) & filled[..., 1:]
        assert (ids[..., :-1][tie] < ids[..., 1:][tie]).all()  # ties: the smaller index first
    assert int(ids_ref(fr, W, H, 1)[2].sum()) == fr[0].size
    # a hand-made set: ties on q inside and across the last slot
    hand = (np.array([7, 3, 9, 5, 1, 2]), np.array([0, 0, 0, 0, 0, 1]), np.array([5, 5, 9, 5, 5, 1], np.uint32))
    i, q, c = ids_ref(hand, 2, 1, 3)
    assert i.tolist() == [[[9, 1, 3], [2, 0xFFFFFFFF, 0xFFFFFFFF]]] and q.tolist() == [[[9, 5, 5], [1, 0, 0]]]
    assert c.tolist() == [[5, 1]] and tie_counts(hand, 2, 1, 3) == (2, 1)
