"""What a depth frame costs beside a colour frame (gs_render_depth).

The bench scene (6M splats, SH3, 1080p, still camera, two frames in flight):
60 untimed frames to leave the idle clocks, then blocks of 20
`render` frames interleaved with blocks of 20 `render_depth` frames, each block
timed with HIP events on the caller's stream, five repeats: median ms per frame
of both paths and their ratio.  Then the same interleaving with stage_timing 2
(one frame in flight at a time is not needed: the events ride in the composite's
own dispatch packet): the composite kernel's median time in both kinds of frame.

  python tools/depth_probe.py [--out profiles/depth/depth_probe.json]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gaussian_splat_amd import scene as S  # noqa: E402
from gaussian_splat_amd.api import InstancedSplatRenderer, Options, default_camera  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--splats", type=int, default=6_000_000)
ap.add_argument("--block", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=60)
args = ap.parse_args()

W, H, N, B = 1920, 1080, args.splats, args.block
scene = S.activate(S.synthetic_raw(N, seed=2, aspect=W / H, rest=True), 3)
cam = default_camera(W, H)
view, proj = cam.getViewMatrix(), cam.getProjectionMatrix()
r = InstancedSplatRenderer(scene, Options(mode="tile", sh_degree=3, crop=False, stage_timing=0, frames_in_flight=2))
r.initialize(0)
out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
depth = torch.empty((H, W), dtype=torch.float32, device="cuda:0")


def colour():
    r.render(view, proj, W, H, out=out)


def with_depth():
    r.render_depth(view, proj, W, H, out=out, depth=depth)


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


for _ in range(args.warmup // 2):
    colour()
    with_depth()
torch.cuda.synchronize()
ref = out.clone()
with_depth()
torch.cuda.synchronize()
assert torch.equal(out, ref), "the depth frame's colour differs from the colour frame"

frames = {"colour": [], "depth": []}
for _ in range(args.repeats):
    frames["colour"].append(block(colour))
    frames["depth"].append(block(with_depth))

# the composite kernel alone, from the events in its own dispatch packet
r.set_stage_timing(2)
kern = {"colour": [], "depth": []}
for _ in range(args.repeats):
    for name, fn in (("colour", colour), ("depth", with_depth)):
        for _ in range(B):
            fn()
        torch.cuda.synchronize()
        _, comp = r.kernel_times(B)
        kern[name].extend(float(x) for x in comp)
r.set_stage_timing(0)

med = {k: statistics.median(v) for k, v in frames.items()}
res = {
    "device": torch.cuda.get_device_name(0),
    "scene": f"{N} splats, SH3, {W}x{H}, still camera, tile rule, two frames in flight",
    "method": f"{args.warmup} untimed frames, then {args.repeats} x (block of {B} colour frames, block of {B} depth frames), "
              "HIP events around each block",
    "ms_per_frame_blocks": frames,
    "ms_per_frame_median": med,
    "depth_over_colour": med["depth"] / med["colour"],
    "depth_below_two_colour_frames": med["depth"] < 2.0 * med["colour"],
    "composite_kernel_ms_median": {k: statistics.median(v) for k, v in kern.items()},
    "composite_kernel_frames": {k: len(v) for k, v in kern.items()},
    "stats_depth_frame": {k: r.last_stats()[k] for k in ("pairs", "pairs_sorted", "records_fetched", "bytes_composite",
                                                         "cut_frame", "open_tiles")},
}
line = json.dumps(res)
print(line)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
