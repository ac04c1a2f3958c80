"""gs_render_features' interface and its CPU reference (no GPU compute is called here)."""
import ctypes as C

import numpy as np
import pytest

from conftest import orbit_views
from depth_ref import depth_from_projection, project_zf
from features_ref import features_from_projection

GS_ERR_INVALID_ARG = 1


def _bits(a, b):
    return int(np.count_nonzero(np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)))


def test_library_exports_gs_render_features(built):
    from gaussian_splat_amd import _lib
    assert "gs_render_features" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "gs_render_features")
    assert _lib.lib().gs_abi_version() == 10  # an addition: the ABI version stays


def test_bad_arguments_are_rejected(built):
    """Null handle, view, proj, out_rgba, out_features or features, a non-positive or
    too large size, channels outside 1..64: GS_ERR_INVALID_ARG with the call's name in
    the error text, also on a handle that was never initialised (the arguments are
    judged first)."""
    from gaussian_splat_amd import InstancedSplatRenderer, Options, _lib
    from gaussian_splat_amd import scene as S
    L = _lib.lib()
    m = np.eye(4, dtype=np.float32).reshape(16)
    fp = m.ctypes.data_as(C.POINTER(C.c_float))
    nofp = C.POINTER(C.c_float)()
    n = 100
    rgba, feats = np.zeros(4 * 4 * 4, np.float32), np.zeros(4 * 4 * 64, np.float32)
    f = np.zeros((n, 64), np.float32)
    R, F, X = rgba.ctypes.data, feats.ctypes.data, f.ctypes.data
    assert L.gs_render_features(None, fp, fp, 4, 4, X, 3, R, F, 0, None) == GS_ERR_INVALID_ARG
    assert "gs_render_features" in _lib.last_error()
    r = InstancedSplatRenderer(S.synthetic_scene(n, seed=1), Options(crop=False))  # (created, not initialised)
    assert r.getPointCount() == n
    good = dict(view=fp, proj=fp, w=4, h=4, x=X, k=3, rgba=R, feats=F)
    bad = [dict(view=nofp), dict(proj=nofp), dict(rgba=None), dict(feats=None), dict(x=None),
           dict(w=0), dict(h=0), dict(w=-3), dict(h=-1), dict(w=65536), dict(h=65536),
           dict(k=0), dict(k=-1), dict(k=65)]
    for case in bad:
        a = {**good, **case}
        st = L.gs_render_features(r._h, a["view"], a["proj"], a["w"], a["h"], a["x"], a["k"], a["rgba"], a["feats"], 0,
                                  None)
        assert st == GS_ERR_INVALID_ARG, (case, st)
        assert "gs_render_features" in _lib.last_error(), (case, _lib.last_error())
    # the limits themselves pass the argument check: the handle's state is judged next
    for k in (1, 64):
        st = L.gs_render_features(r._h, fp, fp, 4, 4, X, k, R, F, 0, None)
        assert st != GS_ERR_INVALID_ARG and "gs_initialize" in _lib.last_error(), (k, st, _lib.last_error())
    r.close()


def test_python_interface_has_render_features(built):
    """The methods exist; a CPU tensor, a 1-D tensor and a float64 tensor (and their numpy
    counterparts of the host call) raise ValueError before the C call."""
    import torch
    from gaussian_splat_amd import InstancedSplatRenderer, Options
    from gaussian_splat_amd import scene as S
    assert callable(InstancedSplatRenderer.render_features) and callable(InstancedSplatRenderer.render_features_host)
    n = 100
    r = InstancedSplatRenderer(S.synthetic_scene(n, seed=1), Options(crop=False))  # (created, not initialised)
    V, P = orbit_views(16, 16, 1)[0]
    for bad in (torch.zeros((n, 3), dtype=torch.float32),  # on the CPU
                torch.zeros((n * 3,), dtype=torch.float32), torch.zeros((n, 3), dtype=torch.float64),
                torch.zeros((n + 1, 3), dtype=torch.float32), torch.zeros((n, 65), dtype=torch.float32),
                torch.zeros((n, 6), dtype=torch.float32)[:, ::2], np.zeros((n, 3), np.float32)):
        with pytest.raises(ValueError):
            r.render_features(V, P, 16, 16, bad)
    for bad in (np.zeros((n * 3,), np.float32), np.zeros((n, 3), np.float64), np.zeros((n + 1, 3), np.float32),
                np.zeros((n, 0), np.float32), np.zeros((n, 65), np.float32), np.zeros((n, 6), np.float32)[:, ::2],
                [[0.0] * 3] * n):
        with pytest.raises(ValueError):
            r.render_features_host(V, P, 16, 16, bad)
    r.close()


@pytest.fixture(scope="module")
def small_frame():
    """test_depth_api.py's frame."""
    from gaussian_splat_amd import scene as S
    W, H = 333, 211
    sc = S.synthetic_scene(6000, seed=11, aspect=W / H)
    sc.scale *= np.float32(3.0)
    V, P = orbit_views(W, H, 1)[0]
    return sc, V, P, W, H, project_zf(sc, V, P, W, H)


@pytest.mark.parametrize("mode", ["tile", "live50"])
def test_one_channel_of_zf_is_the_depth_image(built, small_frame, mode):
    """Depth is the case K = 1, f = zF: features_ref of that column equals depth_ref's
    image bit for bit under both rules (and features_ref's own assertions hold)."""
    sc, V, P, W, H, proj = small_frame
    zf = proj[3]
    depth, colour = depth_from_projection(sc, V, P, W, H, mode, 0, proj)
    feats, colour_f = features_from_projection(sc, V, P, W, H, mode, 0, proj, zf.reshape(-1, 1))
    assert feats.shape == (H, W, 1) and feats.dtype == np.float32
    assert _bits(feats[..., 0], depth) == 0 and _bits(colour_f, colour) == 0
    assert (colour[..., 3] > 0).any() and (colour[..., 3] == 0).any()


def test_reference_channels_are_independent(built, small_frame):
    """A channel's image does not depend on which group of three it is composited in or on
    its neighbours: K = 5 (groups of 3 and 2, zero padded) against the columns one by one."""
    sc, V, P, W, H, proj = small_frame
    rng = np.random.default_rng(3)
    f = rng.standard_normal((proj[2].shape[0], 5)).astype(np.float32)
    all5, _ = features_from_projection(sc, V, P, W, H, "tile", 0, proj, f)
    assert np.isfinite(all5).all() and (all5 != 0).any()
    for k in range(5):
        one, _ = features_from_projection(sc, V, P, W, H, "tile", 0, proj, f[:, k:k + 1])
        assert _bits(all5[..., k], one[..., 0]) == 0, k
