"""What feature passes cost beside a colour frame (gs_render_features).

The bench scene (6M splats, SH3, 1080p, still camera, two frames in flight,
depth_split 0: whole lists in every kind of frame): 60 untimed frames to leave
the idle clocks, then blocks of 20 frames of four kinds, colour,
depth, features K = 4 and features K = 16, interleaved, each block timed with
HIP events on the caller's stream, five repeats: median ms per frame of each
kind and the marginal cost of one four-channel pass, (t_K16 - t_K4) / 3.
Then the yardstick of a pass, the depth composite kernel's own time in these
depth frames (stage_timing 2: the events ride in the composite's dispatch
packet), beside the colour composite's.

  python tools/features_probe.py [--out profiles/features/features_probe.json]

--yardstick-only measures the colour and depth kinds alone (no feature call),
and --root names the tree whose library is loaded: together they measure the
yardstick on another commit's build with this same script.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
ap.add_argument("--yardstick-only", action="store_true")
ap.add_argument("--splats", type=int, default=6_000_000)
ap.add_argument("--block", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=60)
args = ap.parse_args()

sys.path.insert(0, str(Path(args.root).resolve()))
from gaussian_splat_amd import scene as S  # noqa: E402
from gaussian_splat_amd.api import InstancedSplatRenderer, Options, default_camera  # noqa: E402

W, H, N, B = 1920, 1080, args.splats, args.block
scene = S.activate(S.synthetic_raw(N, seed=2, aspect=W / H, rest=True), 3)
cam = default_camera(W, H)
view, proj = cam.getViewMatrix(), cam.getProjectionMatrix()
r = InstancedSplatRenderer(scene, Options(mode="tile", sh_degree=3, crop=False, stage_timing=0, frames_in_flight=2,
                                          depth_split=False))
r.initialize(0)
out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
depth = torch.empty((H, W), dtype=torch.float32, device="cuda:0")

kinds = {"colour": lambda: r.render(view, proj, W, H, out=out),
         "depth": lambda: r.render_depth(view, proj, W, H, out=out, depth=depth)}
if not args.yardstick_only:
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    for K in (4, 16):
        f = torch.randn((r.getPointCount(), K), generator=gen, dtype=torch.float32, device="cuda:0")
        of = torch.empty((H, W, K), dtype=torch.float32, device="cuda:0")
        kinds[f"features_k{K}"] = (lambda f=f, of=of: r.render_features(view, proj, W, H, f, out=out, out_features=of))


def block(fn):
    """ms per frame of B frames, HIP events around the block on the caller's stream."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(B):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / B


for _ in range(max(args.warmup // len(kinds), 1)):
    for fn in kinds.values():
        fn()
torch.cuda.synchronize()
kinds["colour"]()
torch.cuda.synchronize()
ref = out.clone()
for name, fn in kinds.items():
    fn()
    torch.cuda.synchronize()
    assert torch.equal(out, ref), f"the {name} frame's colour differs from the colour frame"

frames = {k: [] for k in kinds}
for _ in range(args.repeats):
    for name, fn in kinds.items():
        frames[name].append(block(fn))
stats = {name: None for name in kinds}
for name, fn in kinds.items():
    fn()
    stats[name] = {k: r.last_stats()[k] for k in ("pairs", "pairs_sorted", "records_fetched", "bytes_composite",
                                                  "cut_frame", "open_tiles")}

# the composite kernel alone, from the events in its own dispatch packet (in a feature frame
# they ride in the colour composite's packet: the feature passes are not in this figure)
r.set_stage_timing(2)
kern = {"colour": [], "depth": []}
for _ in range(args.repeats):
    for name in kern:
        for _ in range(B):
            kinds[name]()
        torch.cuda.synchronize()
        _, comp = r.kernel_times(B)
        kern[name].extend(float(x) for x in comp)
r.set_stage_timing(0)

med = {k: statistics.median(v) for k, v in frames.items()}
kmed = {k: statistics.median(v) for k, v in kern.items()}
res = {
    "device": torch.cuda.get_device_name(0),
    "scene": f"{N} splats, SH3, {W}x{H}, still camera, tile rule, two frames in flight, depth_split 0",
    "method": f"{args.warmup} untimed frames, then {args.repeats} x (a block of {B} frames of each kind), "
              "HIP events around each block",
    "ms_per_frame_blocks": frames,
    "ms_per_frame_median": med,
    "composite_kernel_ms_median": kmed,
    "composite_kernel_frames": {k: len(v) for k, v in kern.items()},
    "yardstick_depth_composite_kernel_ms": kmed["depth"],
    "stats": stats,
}
if not args.yardstick_only:
    pass_ms = (med["features_k16"] - med["features_k4"]) / 3.0
    res["marginal_pass_ms"] = pass_ms
    res["first_pass_ms"] = med["features_k4"] - med["colour"]
    res["marginal_pass_over_yardstick"] = pass_ms / kmed["depth"]
line = json.dumps(res)
print(line)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
