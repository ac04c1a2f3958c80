"""gs_render_depth's interface and its CPU reference (no GPU compute is called here)."""
import ctypes as C

import numpy as np
import pytest

from conftest import orbit_views
from depth_ref import depth_from_projection, project_zf

GS_ERR_INVALID_ARG = 1


def test_library_exports_gs_render_depth(built):
    from gaussian_splat_amd import _lib
    assert "gs_render_depth" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "gs_render_depth")
    assert _lib.lib().gs_abi_version() == 10  # an addition: the ABI version stays


def test_bad_arguments_are_rejected(built):
    """Null handle, null out_depth, zero and negative sizes: GS_ERR_INVALID_ARG,
    also on a handle that was never initialised (the arguments are judged first)."""
    from gaussian_splat_amd import InstancedSplatRenderer, Options, _lib
    from gaussian_splat_amd import scene as S
    L = _lib.lib()
    m = np.eye(4, dtype=np.float32).reshape(16)
    fp = m.ctypes.data_as(C.POINTER(C.c_float))
    rgba, depth = np.zeros(4 * 4 * 4, np.float32), np.zeros(4 * 4, np.float32)
    assert L.gs_render_depth(None, fp, fp, 4, 4, rgba.ctypes.data, depth.ctypes.data, 0, None) == GS_ERR_INVALID_ARG
    r = InstancedSplatRenderer(S.synthetic_scene(100, seed=1), Options(crop=False))  # (created, not initialised)
    for w, h, d in ((4, 4, None), (0, 4, depth.ctypes.data), (4, 0, depth.ctypes.data), (-3, 4, depth.ctypes.data),
                    (4, -1, depth.ctypes.data)):
        assert L.gs_render_depth(r._h, fp, fp, w, h, rgba.ctypes.data, d, 0, None) == GS_ERR_INVALID_ARG, (w, h, d)
        assert "gs_render_depth" in _lib.last_error()
    r.close()


def test_python_interface_has_render_depth(built):
    from gaussian_splat_amd import InstancedSplatRenderer
    assert callable(InstancedSplatRenderer.render_depth) and callable(InstancedSplatRenderer.render_depth_host)


@pytest.fixture(scope="module")
def small_frame():
    from gaussian_splat_amd import scene as S
    W, H = 333, 211
    sc = S.synthetic_scene(6000, seed=11, aspect=W / H)
    sc.scale *= np.float32(3.0)
    V, P = orbit_views(W, H, 1)[0]
    return sc, V, P, W, H, project_zf(sc, V, P, W, H)


@pytest.mark.parametrize("mode", ["tile", "live50"])
def test_depth_ref_is_self_consistent(built, small_frame, mode):
    """depth_ref's own assertions (the record composite is the oracle's frame; G, B
    and A unchanged by the depth in the red channel) hold, and the image is a depth:
    zero exactly where nothing lands, positive and finite elsewhere."""
    sc, V, P, W, H, proj = small_frame
    depth, colour = depth_from_projection(sc, V, P, W, H, mode, 0, proj)
    assert depth.shape == (H, W) and depth.dtype == np.float32 and np.isfinite(depth).all()
    a = colour[..., 3]
    assert (a > 0).any() and (a == 0).any()
    assert (depth[a == 0] == 0.0).all() and (depth[a > 0] > 0.0).all()


def test_tile_depth_over_alpha_lies_within_the_visible_depths(built, small_frame):
    """Tile rule: D = sum zF_i w_i and A = sum w_i over the same weights, so D / A
    is a weighted mean of the visible splats' zF: inside their range (1e-5 relative:
    fp32 rounding of the two sums)."""
    sc, V, P, W, H, proj = small_frame
    depth, colour = depth_from_projection(sc, V, P, W, H, "tile", 0, proj)
    _, _, ntiles, zf = proj
    lo, hi = float(zf[ntiles > 0].min()), float(zf[ntiles > 0].max())
    a = colour[..., 3].astype(np.float64)
    q = depth.astype(np.float64)[a > 0] / a[a > 0]
    print(f"D/A in [{q.min():.4f}, {q.max():.4f}], visible zF in [{lo:.4f}, {hi:.4f}]")
    assert q.min() >= lo * (1 - 1e-5) and q.max() <= hi * (1 + 1e-5)
