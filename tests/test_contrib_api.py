"""gs_render_contrib's interface and its CPU reference (no GPU compute is called here)."""
import ctypes as C

import numpy as np
import pytest

from conftest import orbit_views
from contrib_ref import contrib_fragments, contrib_totals, quantise, single_splat_totals
from depth_ref import project_zf

GS_ERR_INVALID_ARG = 1


def test_library_exports_gs_render_contrib(built):
    from gaussian_splat_amd import _lib
    assert "gs_render_contrib" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "gs_render_contrib")
    assert _lib.lib().gs_abi_version() == 10  # an addition: the ABI version stays


def test_bad_arguments_are_rejected(built):
    """Null handle, view, proj, out_rgba or any of the three arrays, a size outside
    1..65535, accumulate or is_device outside {0, 1}: GS_ERR_INVALID_ARG with the call's
    name in the error text, also on a handle that was never initialised (the arguments are
    judged first).  Good arguments get past the check to the handle's state."""
    from gaussian_splat_amd import InstancedSplatRenderer, Options, _lib
    from gaussian_splat_amd import scene as S
    L = _lib.lib()
    m = np.eye(4, dtype=np.float32).reshape(16)
    fp = m.ctypes.data_as(C.POINTER(C.c_float))
    nofp = C.POINTER(C.c_float)()
    n = 100
    rgba = np.zeros(4 * 4 * 4, np.float32)
    s, c, x = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    mask = np.ones(16, np.uint8)
    R, S_, C_, X, M = rgba.ctypes.data, s.ctypes.data, c.ctypes.data, x.ctypes.data, mask.ctypes.data
    assert L.gs_render_contrib(None, fp, fp, 4, 4, None, R, S_, C_, X, 0, 0, None) == GS_ERR_INVALID_ARG
    assert "gs_render_contrib" in _lib.last_error()
    r = InstancedSplatRenderer(S.synthetic_scene(n, seed=1), Options(crop=False))  # (created, not initialised)
    assert r.getPointCount() == n
    good = dict(view=fp, proj=fp, w=4, h=4, mask=None, rgba=R, s=S_, c=C_, x=X, acc=0, dev=0)

    def call(a):
        return L.gs_render_contrib(r._h, a["view"], a["proj"], a["w"], a["h"], a["mask"], a["rgba"], a["s"], a["c"],
                                   a["x"], a["acc"], a["dev"], None)

    bad = [dict(view=nofp), dict(proj=nofp), dict(rgba=None), dict(s=None), dict(c=None), dict(x=None),
           dict(w=0), dict(h=0), dict(w=-3), dict(h=-1), dict(w=65536), dict(h=65536),
           dict(acc=2), dict(acc=-1), dict(dev=2), dict(dev=-1)]
    for case in bad:
        st = call({**good, **case})
        assert st == GS_ERR_INVALID_ARG, (case, st)
        assert "gs_render_contrib" in _lib.last_error(), (case, _lib.last_error())
    # good arguments pass the argument check: the handle's state is judged next
    for case in (dict(), dict(mask=M), dict(acc=1), dict(dev=1), dict(w=65535, h=1), dict(w=1, h=65535)):
        st = call({**good, **case})
        assert st != GS_ERR_INVALID_ARG and "gs_initialize" in _lib.last_error(), (case, st, _lib.last_error())
    assert not s.any() and not c.any() and not x.any() and not rgba.any()
    r.close()


def test_python_interface_has_render_contrib(built):
    """The methods exist; a CPU tensor, a wrong dtype, a wrong shape and a non-contiguous
    mask (and their numpy counterparts of the host call) raise ValueError before the C call."""
    import torch
    from gaussian_splat_amd import InstancedSplatRenderer, Options
    from gaussian_splat_amd import scene as S
    assert callable(InstancedSplatRenderer.render_contrib) and callable(InstancedSplatRenderer.render_contrib_host)
    n = 100
    r = InstancedSplatRenderer(S.synthetic_scene(n, seed=1), Options(crop=False))  # (created, not initialised)
    V, P = orbit_views(16, 16, 1)[0]
    W, H = 16, 8
    for kw in (dict(mask=torch.ones((H, W), dtype=torch.uint8)),  # on the CPU
               dict(mask=torch.ones((H, W), dtype=torch.float32)), dict(mask=torch.ones((W, H), dtype=torch.uint8)),
               dict(mask=torch.ones((H, 2 * W), dtype=torch.uint8)[:, ::2]), dict(mask=np.ones((H, W), np.uint8)),
               dict(sum=torch.zeros(n, dtype=torch.int64)),  # on the CPU
               dict(sum=torch.zeros(n, dtype=torch.int32)), dict(count=torch.zeros(n, dtype=torch.int64)),
               dict(max=torch.zeros(n, dtype=torch.float32)), dict(sum=torch.zeros(n + 1, dtype=torch.int64)),
               dict(count=torch.zeros(2 * n, dtype=torch.int32)[::2]), dict(accumulate=True),
               dict(accumulate=True, sum=torch.zeros(n, dtype=torch.int64))):
        with pytest.raises(ValueError):
            r.render_contrib(V, P, W, H, **kw)
    for kw in (dict(mask=np.ones((H, W), np.float32)), dict(mask=np.ones((W, H), np.uint8)),
               dict(mask=np.ones((H, 2 * W), np.uint8)[:, ::2]), dict(mask=[[1] * W] * H),
               dict(sum=np.zeros(n, np.int64)), dict(count=np.zeros(n, np.uint64)), dict(max=np.zeros(n, np.float32)),
               dict(sum=np.zeros(n + 1, np.uint64)), dict(count=np.zeros(2 * n, np.uint32)[::2]),
               dict(accumulate=True)):
        with pytest.raises(ValueError):
            r.render_contrib_host(V, P, W, H, **kw)
    r.close()


def test_quantise():
    """q: truncation, clamped to 0 .. 2^24, NaN to 0, below 2^-24 to 0."""
    w = np.array([0.0, -0.0, -1.0, 1.0, 2.0, np.inf, -np.inf, np.nan, 2.0 ** -24, 2.0 ** -25, 0.5, 1.0 - 2.0 ** -24,
                  3.0 * 2.0 ** -25, 1e-45], np.float32)
    want = [0, 0, 0, 1 << 24, 1 << 24, 1 << 24, 0, 0, 1, 0, 1 << 23, (1 << 24) - 1, 1, 0]
    assert quantise(w).tolist() == want


@pytest.fixture(scope="module")
def tiny_frame():
    from gaussian_splat_amd import scene as S
    W, H = 96, 64
    sc = S.synthetic_scene(300, seed=5, aspect=W / H)
    sc.scale *= np.float32(3.0)
    V, P = orbit_views(W, H, 1)[0]
    return sc, V, P, W, H, project_zf(sc, V, P, W, H)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mode", ["tile", "live50"])
def test_reference_agrees_with_single_splat_composites(built, tiny_frame, mode, masked):
    """contrib_ref's sets against one indicator composite per splat, every splat of a
    300-splat scene at 96 x 64, both rules, with and without a random mask."""
    sc, V, P, W, H, proj = tiny_frame
    rec, dkey = proj[0], proj[1]
    n = rec.shape[0]
    mask = (np.random.default_rng(4).random((H, W)) < 0.6).astype(np.uint8) if masked else None
    fr = contrib_fragments(sc, V, P, W, H, mode, 0, proj)
    s, c, m = contrib_totals(fr, n, mask)
    info = fr[4]
    assert 1 < info["sets"] < n and info["composites"] == (info["sets"] + 2) // 3
    assert s.dtype == np.uint64 and c.dtype == np.uint32 and m.dtype == np.uint32
    one = single_splat_totals(rec, dkey, W, H, mode, range(n), mask)
    for i in range(n):
        assert (int(s[i]), int(c[i]), int(m[i])) == one[i], (i, one[i])
    assert (c > 0).sum() > 50 and (c == 0).any()
    assert (m <= (1 << 24)).all() and (s >= m).all() and ((c == 0) == (s == 0)).all()
    if masked:  # a mask only removes
        s0, c0, m0 = contrib_totals(fr, n, None)
        assert (s <= s0).all() and (c <= c0).all() and (m <= m0).all() and (s < s0).any()
