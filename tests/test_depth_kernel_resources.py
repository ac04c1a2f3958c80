"""Register, scratch and LDS budgets of the depth composites (composite_depth.hip;
CPU: hipcc cross-compiles gfx950), by the method of test_kernel_resources.py.

The depth kernels carry one more accumulator per pixel (two in the strip kernel),
the staged depth of each record in flight and the owner lane's gathered depth, so
they are built for 6 waves per SIMD (the 80-VGPR class) instead of the colour
kernels' 8.  Limits: no VGPR spill; scratch no larger than the colour kernel's
limit of the same pass (8 B pass 0, 16 B passes 1 and 2); the 80-SGPR allocation
class (TotalSGPRs <= 64: they share SIMDs with the preprocess in the pipelined
frame, composite.hip GS_COMPOSITE_SGPRS); 16 KB of LDS; at least 6 waves per SIMD.
The committed build measures, all passes and both rules: tile kernel 68-69 VGPRs
(7 waves), strip kernel 78 VGPRs (6 waves), 60 SGPRs, no scratch, 14,608 and
15,664 B of LDS."""
import pytest

from test_kernel_resources import _one, _resources


@pytest.fixture(scope="module")
def depth_res():
    return _resources("composite_depth.hip")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("pass_", [0, 1, 2])
@pytest.mark.parametrize("kernel", ["composite_depth_kernel", "composite_strip_depth_kernel"])
def test_depth_composite_budget(depth_res, kernel, pass_, mode):
    r = _one(depth_res, rf"{kernel}ILi{mode}ELi{pass_}EE")
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] <= (8 if pass_ == 0 else 16), r
    assert r["TotalSGPRs"] <= 64, r
    assert r["LDS Size"] <= 16 * 1024, r
    assert r["Occupancy"] >= 6 and r["VGPRs"] <= 80, r


def test_zf_plane_kernel_is_trivial(depth_res):
    r = _one(depth_res, r"zf_plane_kernel")
    assert r["ScratchSize"] == 0 and r["LDS Size"] == 0 and r["Occupancy"] == 8, r
