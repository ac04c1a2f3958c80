"""Register, scratch and LDS budgets of the feature composites (composite_features.hip;
CPU: hipcc cross-compiles gfx950), by the method of test_kernel_resources.py.

The feature kernels are the depth kernels' register class: T and four accumulators
per pixel (eight in the strip kernel), the staged values of each record in flight
and the owner lane's four gathered values (three registers over the depth kernels'
one).  Limits: no VGPR spill; at most 8 B of scratch (the colour composite's pass-0
limit); the 80-SGPR allocation class (TotalSGPRs <= 64: the passes run beside the
next frame's preprocess in the pipelined frame, composite.hip GS_COMPOSITE_SGPRS);
16 KB of LDS; at least 5 waves per SIMD, and what the committed build reaches where
that is more: 7 for the tile kernel, 6 for the strip kernel.
The committed build measures, both rules, by gather / store form (16-B or dwords):
  composite_feat_kernel        16-B gather 69 VGPRs, dword gather 70 (7 waves),
                               60 SGPRs (2-3 spilled to VGPR lanes with the dword
                               gather), no scratch, 14,608 B of LDS
  composite_strip_feat_kernel  16-B gather 78 VGPRs, dword gather 79 (6 waves),
                               60 SGPRs (6-7 spilled to VGPR lanes with the dword
                               gather), no scratch, 15,664 B of LDS"""
import pytest

from test_kernel_resources import _one, _resources


@pytest.fixture(scope="module")
def feat_res():
    return _resources("composite_features.hip")


@pytest.mark.parametrize("vout", [0, 1])
@pytest.mark.parametrize("vin", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kernel,waves", [("composite_feat_kernel", 7), ("composite_strip_feat_kernel", 6)])
def test_feature_composite_budget(feat_res, kernel, waves, mode, vin, vout):
    r = _one(feat_res, rf"{kernel}ILi{mode}ELb{vin}ELb{vout}EE")
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize"] <= 8, r
    assert r["TotalSGPRs"] <= 64, r
    assert r["LDS Size"] <= 16 * 1024, r
    assert r["Occupancy"] >= 5, r
    assert r["Occupancy"] >= waves and r["VGPRs"] <= 512 // waves // 8 * 8, r  # (the committed build's class)
