"""Register, scratch and LDS budgets of the contrib composites (composite_contrib.hip;
CPU: hipcc cross-compiles gfx950), by the method of test_kernel_resources.py.

The contrib kernels carry T per pixel, the pixel's weight scale and no accumulator, so
they are the colour kernels' register class with room to spare; the wave reduction and
the three atomics of a (record, wave) need no LDS beyond the bodies' own.  Limits: no
VGPR spill; at most 8 B of scratch (the colour composite's pass-0 limit); the 80-SGPR
allocation class (TotalSGPRs <= 64: the pass runs beside the next frame's preprocess in
the pipelined frame, composite.hip GS_COMPOSITE_SGPRS); 16 KB of LDS; at least 5 waves
per SIMD, and the 8 the committed build reaches.
The committed build measures, both rules alike:
  composite_contrib_kernel        57 VGPRs (8 waves), 58 SGPRs, none spilled, no scratch,
                                  14,608 B of LDS
  composite_strip_contrib_kernel  56 VGPRs (8 waves), 59 SGPRs, none spilled, no scratch,
                                  14,640 B of LDS"""
import pytest

from test_kernel_resources import _one, _resources


@pytest.fixture(scope="module")
def contrib_res():
    return _resources("composite_contrib.hip")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kernel,waves", [("composite_contrib_kernel", 8), ("composite_strip_contrib_kernel", 8)])
def test_contrib_composite_budget(contrib_res, kernel, waves, mode):
    r = _one(contrib_res, rf"\d{kernel}ILi{mode}EE")
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] <= 8, r
    assert r["TotalSGPRs"] <= 64, r
    assert r["LDS Size"] <= 16 * 1024, r
    assert r["Occupancy"] >= 5, r
    assert r["Occupancy"] >= waves and r["VGPRs"] <= 512 // waves // 8 * 8, r  # (the committed build's class)


def test_every_contrib_instance_is_covered(contrib_res):
    """Both kernels, both rules, and nothing else in the file."""
    assert len(contrib_res) == 4, sorted(contrib_res)
