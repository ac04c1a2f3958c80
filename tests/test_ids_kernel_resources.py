"""Register, scratch and LDS budgets of the ids composites (composite_ids.hip; CPU: hipcc
cross-compiles gfx950), by the method of test_kernel_resources.py.

The ids kernels are the contrib kernels without the wave reduction and the atomics, plus
K (q, id) pairs and a counter per pixel in VGPRs: 2 K + 1 registers in the tile body (one
pixel per lane), 4 K + 2 in the strip body (two).  Limits, test_contrib_kernel_resources.py's:
no VGPR spill; at most 8 B of scratch; the 80-SGPR allocation class (TotalSGPRs <= 64);
16 KB of LDS; at least 5 waves per SIMD, and the class each instance of the committed build
reaches (kWaves per instance: ids_waves(), composite_ids.hip).
The committed build measures, both rules alike, none spilled, no scratch:
  composite_ids_kernel        K = 1: 60 VGPRs (8 waves), 60 SGPRs   14,608 B of LDS
                              K = 2: 62 VGPRs (8 waves), 60 SGPRs
                              K = 4: 63 VGPRs (8 waves), 59 SGPRs
  composite_strip_ids_kernel  K = 1: 71 VGPRs (7 waves), 60 SGPRs   14,640 B of LDS
                              K = 2: 72 VGPRs (7 waves), 60 SGPRs
                              K = 4: 93 VGPRs (5 waves), 60 SGPRs
(the strip kernel at K = 4 spills 9 VGPRs when built for 6 waves and 25 for 8)."""
import pytest

from test_kernel_resources import _one, _resources

WAVES = {("composite_ids_kernel", 1): 8, ("composite_ids_kernel", 2): 8, ("composite_ids_kernel", 4): 8,
         ("composite_strip_ids_kernel", 1): 7, ("composite_strip_ids_kernel", 2): 7, ("composite_strip_ids_kernel", 4): 5}


@pytest.fixture(scope="module")
def ids_res():
    return _resources("composite_ids.hip")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kernel,k", sorted(WAVES))
def test_ids_composite_budget(ids_res, kernel, k, mode):
    waves = WAVES[kernel, k]
    r = _one(ids_res, rf"\d{kernel}ILi{mode}ELi{k}EE")
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] <= 8, r
    assert r["TotalSGPRs"] <= 64, r
    assert r["LDS Size"] <= 16 * 1024, r
    assert r["Occupancy"] >= 5, r
    assert r["Occupancy"] >= waves and r["VGPRs"] <= 512 // waves // 8 * 8, r  # (the committed build's class)


def test_every_ids_instance_is_covered(ids_res):
    """Both kernels, both rules, K = 1, 2 and 4, and nothing else in the file."""
    assert len(ids_res) == 2 * 2 * 3, sorted(ids_res)
