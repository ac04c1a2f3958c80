"""What the ids pass costs beside a colour frame (gs_render_ids).

The bench scene (6M splats, SH3, 1080p, still camera, two frames in flight,
depth_split 0: whole lists in every kind of frame): 60 untimed frames to leave
the idle clocks, then blocks of 20 frames of each kind, colour,
contrib, ids with 1 slot and ids with 4 slots, interleaved, each block timed
with HIP events on the caller's stream, five repeats: median ms per frame of
each kind and the marginal cost of each pass, t_kind - t_colour.

  python tools/ids_probe.py [--out profiles/ids/ids_probe.json]

--root names the tree whose library is loaded; with a tree that has no
gs_render_ids (the parent commit's build) the ids kinds are left out and the
colour and contrib frames alone are measured, with this same script.
--only KIND runs frames of one kind alone (for a counters-only profiler run of
that kind's kernels).
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
ap.add_argument("--splats", type=int, default=6_000_000)
ap.add_argument("--block", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=60)
ap.add_argument("--only", default=None)
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
n = r.getPointCount()
cs = torch.empty((n,), dtype=torch.int64, device="cuda:0")
cc = torch.empty((n,), dtype=torch.int32, device="cuda:0")
cm = torch.empty((n,), dtype=torch.int32, device="cuda:0")

kinds = {"colour": lambda: r.render(view, proj, W, H, out=out),
         "contrib": lambda: r.render_contrib(view, proj, W, H, out=out, sum=cs, count=cc, max=cm)}
has_ids = hasattr(r, "render_ids")
if has_ids:
    bufs = {s: [torch.empty((H, W, s), dtype=torch.int32, device="cuda:0") for _ in range(2)] for s in (1, 4)}
    cnt = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
    for s in (1, 4):
        kinds[f"ids_{s}"] = (lambda s=s: r.render_ids(view, proj, W, H, slots=s, out=out, ids=bufs[s][0], q=bufs[s][1],
                                                      count=cnt))
if args.only:
    kinds = {"colour": kinds["colour"], args.only: kinds[args.only]}


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
stats = {}
for name, fn in kinds.items():
    fn()
    stats[name] = {k: r.last_stats()[k] for k in ("pairs", "pairs_sorted", "records_fetched", "bytes_composite",
                                                  "cut_frame", "open_tiles")}

med = {k: statistics.median(v) for k, v in frames.items()}
res = {
    "device": torch.cuda.get_device_name(0),
    "scene": f"{N} splats, SH3, {W}x{H}, still camera, tile rule, two frames in flight, depth_split 0",
    "method": f"{args.warmup} untimed frames, then {args.repeats} x (a block of {B} frames of each kind), "
              "HIP events around each block",
    "ms_per_frame_blocks": frames,
    "ms_per_frame_median": med,
    "stats": stats,
}
for k in med:
    if k != "colour":
        res[f"{k}_pass_ms"] = med[k] - med["colour"]
if has_ids and "ids_4" in kinds:
    torch.cuda.synchronize()
    kinds["ids_4"]()
    torch.cuda.synchronize()
    c = cnt.to(torch.int64)
    res["pixels_without_candidate"] = int((c == 0).sum())
    res["pixels_with_more_than_4"] = int((c > 4).sum())
    res["candidates_per_pixel_mean"] = float(c.double().mean())
line = json.dumps(res)
print(line)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
