"""Register, scratch and LDS budgets of the scene re-indexing kernels (select.hip; CPU: hipcc
cross-compiles gfx950), by the method of test_kernel_resources.py.

The compaction kernels keep four 64-bit ballots per wave and exchange four wave totals through
16 B of LDS; the gather holds every plane entry of its splat in registers between its loads and
its stores (3 float4 + 1 float2 + NP4 float4 + the tail: 14 + 4 NP4 + 1 data VGPRs) and uses no
LDS.  Limits: no VGPR spill, no scratch, 16 B of LDS in the compaction kernels and none in the
gather, and the occupancy class each kernel of the committed build reaches.
The committed build measures, none spilled, no scratch:
  select_count_kernel             8 VGPRs, 22 SGPRs, 16 B of LDS, 8 waves
  select_scan_kernel             27 VGPRs, 44 SGPRs, 16 B of LDS, 8 waves
  select_emit_kernel             16 VGPRs, 24 SGPRs, 16 B of LDS, 8 waves
  select_gather_kernel  SH 0     24 VGPRs, 22 SGPRs, no LDS,      8 waves
                        SH 1     39 VGPRs, 30 SGPRs               8 waves
                        SH 2     56 VGPRs, 24 SGPRs               8 waves
                        SH 3     67 VGPRs, 26 SGPRs               7 waves
(SH 3 moves 236 B per splat: 59 data registers live between the loads and the stores.)"""
import pytest

from test_kernel_resources import _one, _resources

# kernel pattern -> (waves per SIMD of the committed build, LDS bytes allowed)
KERNELS = {r"select_count_kernelE": (8, 16), r"select_scan_kernelE": (8, 16), r"select_emit_kernelE": (8, 16),
           r"select_gather_kernelILi0ELb0EE": (8, 0), r"select_gather_kernelILi2ELb1EE": (8, 0),
           r"select_gather_kernelILi6ELb0EE": (8, 0), r"select_gather_kernelILi11ELb1EE": (7, 0)}


@pytest.fixture(scope="module")
def select_res():
    return _resources("select.hip")


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_select_kernel_budget(select_res, kernel):
    waves, lds = KERNELS[kernel]
    r = _one(select_res, kernel)
    assert r["VGPRs Spill"] == 0 and r.get("SGPRs Spill", 0) == 0, r
    assert r["ScratchSize"] == 0, r
    assert r["LDS Size"] <= lds, r
    assert r["Occupancy"] >= waves and r["VGPRs"] <= 512 // waves // 8 * 8, r  # (the committed build's class)


def test_every_select_kernel_is_covered(select_res):
    """The three compaction kernels and the gather at SH 0..3, and nothing else in the file."""
    assert len(select_res) == len(KERNELS), sorted(select_res)
