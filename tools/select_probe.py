"""What re-indexing the scene on the device costs (gs_select / gs_prune).

The bench scene (6M splats, SH3) on one initialised handle.  Three calls are
timed, host wall clock around each (both calls are synchronous for the host and
return with the host and the device planes in place): gs_prune keeping a seeded
half, gs_select with the identity and gs_select with a seeded random
permutation.  Between repeats an untimed gs_select with a repeating list brings
the handle back to N splats, so every repeat moves the same bytes.  Two
baselines in the same run:
  (a) a device-to-device hipMemcpy of the same planes (the rate a gather cannot
      beat), HIP's own copy, timed with a device synchronise on either side;
  (b) the route a caller had before: gs_get_scene -> numpy indexing ->
      gs_create_from_soa -> gs_initialize, for the same half.
A few untimed rounds first (clocks, allocator); then --repeats rounds; the JSON
holds every sample, the medians and the spread.

  python tools/select_probe.py [--out profiles/select/select_probe.json]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--splats", type=int, default=6_000_000)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--route-repeats", type=int, default=2)
args = ap.parse_args()

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gaussian_splat_amd import scene as S  # noqa: E402
from gaussian_splat_amd.api import InstancedSplatRenderer, Options  # noqa: E402

N, SH = args.splats, 3
K = 15  # sh_coeffs(3)
BYTES_PER_SPLAT = 56 + 12 * K  # every plane entry of a splat
opts = dict(mode="tile", sh_degree=SH, crop=False)
scene = S.activate(S.synthetic_raw(N, seed=2, aspect=16 / 9, rest=True), SH)
r = InstancedSplatRenderer(scene, Options(**opts))
r.initialize(0)
rng = np.random.default_rng(5)
keep = torch.from_numpy((rng.random(N) < 0.5).astype(np.uint8)).cuda()
kept = int(keep.sum())
identity = torch.arange(N, dtype=torch.int32, device="cuda:0")
perm = torch.from_numpy(rng.permutation(N).astype(np.int32)).cuda()
torch.cuda.synchronize()


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def regrow():
    """Back to N splats after a prune: each kept splat about twice (untimed)."""
    m = r.getPointCount()
    r.select((torch.arange(N, dtype=torch.int64, device="cuda:0") * m // N).to(torch.int32))
    assert r.getPointCount() == N


samples = {"prune_half": [], "select_identity": [], "select_permutation": []}
for k in range(args.warmup + args.repeats):
    t_prune = wall(lambda: r.prune(keep))
    assert r.getPointCount() == kept
    regrow()
    t_id = wall(lambda: r.select(identity))
    t_perm = wall(lambda: r.select(perm))
    if k >= args.warmup:
        samples["prune_half"].append(t_prune)
        samples["select_identity"].append(t_id)
        samples["select_permutation"].append(t_perm)

# (a) HIP's device-to-device copy of the same planes: p0, p1, p2, p3, the 11 SH planes, the tail
# (the HIP runtime torch has loaded: its tensors are that runtime's allocations)
loaded = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln and "torch" in ln]
hip = C.CDLL(loaded[0] if loaded else "libamdhip64.so")
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipMemcpy.restype = C.c_int
planes = [16, 16, 16, 8, 11 * 16, 4]
src = [torch.empty(N * b, dtype=torch.uint8, device="cuda:0") for b in planes]
dst = [torch.empty(N * b, dtype=torch.uint8, device="cuda:0") for b in planes]
assert sum(planes) == BYTES_PER_SPLAT


def copy_planes():
    for s, d in zip(src, dst):
        assert hip.hipMemcpy(d.data_ptr(), s.data_ptr(), s.numel(), 3) == 0  # hipMemcpyDeviceToDevice


for k in range(args.warmup + args.repeats):
    t = wall(copy_planes)
    if k >= args.warmup:
        samples.setdefault("copy_d2d", []).append(t)
del src, dst

# (b) the route through the host, for the same half
half = np.flatnonzero(keep.cpu().numpy())
for k in range(args.route_repeats):
    t0 = time.perf_counter()
    sc = r.scene()
    t1 = time.perf_counter()
    sub = sc.subset(half)
    t2 = time.perf_counter()
    r2 = InstancedSplatRenderer(sub, Options(**opts))
    t3 = time.perf_counter()
    r2.initialize(0)
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    samples.setdefault("host_route", []).append((t4 - t0) * 1e3)
    samples.setdefault("host_route_parts", []).append(
        {"get_scene": (t1 - t0) * 1e3, "index": (t2 - t1) * 1e3, "create_from_soa": (t3 - t2) * 1e3,
         "initialize": (t4 - t3) * 1e3})
    r2.close()
    del sc, sub

names = ["prune_half", "select_identity", "select_permutation", "copy_d2d", "host_route"]
med = {k: statistics.median(samples[k]) for k in names}
moved = {"prune_half": kept, "select_identity": N, "select_permutation": N, "copy_d2d": N}
res = {
    "device": torch.cuda.get_device_name(0),
    "scene": f"{N} splats, SH3 ({BYTES_PER_SPLAT} B per splat in the planes); the half keeps {kept}",
    "method": f"host wall clock around each synchronous call, {args.warmup} untimed rounds, then {args.repeats}; "
              f"the host route {args.route_repeats} times",
    "ms": samples,
    "ms_median": med,
    "ms_min_max": {k: [min(samples[k]), max(samples[k])] for k in names},
    "gb_per_s_read_plus_write": {k: 2 * moved[k] * BYTES_PER_SPLAT / med[k] / 1e6 for k in moved},
    "prune_over_host_route": med["prune_half"] / med["host_route"],
    "select_identity_over_copy": med["select_identity"] / med["copy_d2d"],
    "select_permutation_over_copy": med["select_permutation"] / med["copy_d2d"],
}
print(json.dumps(res))
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
