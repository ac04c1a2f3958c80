"""What the contrib pass costs beside a colour frame (gs_render_contrib).

The bench scene (6M splats, SH3, 1080p, still camera, two frames in flight,
depth_split 0: whole lists in every kind of frame): 60 untimed frames to leave
the idle clocks, then blocks of 20 frames of four kinds, colour,
features K = 4, contrib without a mask and contrib with a mask, interleaved,
each block timed with HIP events on the caller's stream, five repeats: median
ms per frame of each kind, the marginal cost of the contrib pass, t_contrib -
t_colour, and of one four-channel feature pass, t_K4 - t_colour, the yardstick.

  python tools/contrib_probe.py [--out profiles/contrib/contrib_probe.json]

--root names the tree whose library is loaded; with a tree that has no
gs_render_contrib (the parent commit's build) the contrib kinds are left out
and the yardstick alone is measured, with this same script.  --yardstick
names such a run's output: its marginal feature pass is then the ratio's
denominator.
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
ap.add_argument("--yardstick", default=None)
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
gen = torch.Generator(device="cuda:0").manual_seed(5)
f = torch.randn((r.getPointCount(), 4), generator=gen, dtype=torch.float32, device="cuda:0")
of = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")

kinds = {"colour": lambda: r.render(view, proj, W, H, out=out),
         "features_k4": lambda: r.render_features(view, proj, W, H, f, out=out, out_features=of)}
has_contrib = hasattr(r, "render_contrib")
if has_contrib:
    n = r.getPointCount()
    cs = torch.empty((n,), dtype=torch.int64, device="cuda:0")
    cc = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    cm = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    mask = (torch.rand((H, W), generator=gen, device="cuda:0") < 0.5).to(torch.uint8)
    kinds["contrib"] = lambda: r.render_contrib(view, proj, W, H, out=out, sum=cs, count=cc, max=cm)
    kinds["contrib_mask"] = lambda: r.render_contrib(view, proj, W, H, mask=mask, out=out, sum=cs, count=cc, max=cm)


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
    "feature_pass_ms": med["features_k4"] - med["colour"],
    "stats": stats,
}
if has_contrib:
    torch.cuda.synchronize()
    kinds["contrib"]()
    torch.cuda.synchronize()
    res["splats_with_weight"] = int((cc != 0).sum())
    res["weight_total_pixels"] = float(cs.double().sum() / 2.0 ** 24)
    res["contrib_pass_ms"] = med["contrib"] - med["colour"]
    res["contrib_mask_pass_ms"] = med["contrib_mask"] - med["colour"]
    yard = res["feature_pass_ms"]
    if args.yardstick:
        yard = json.loads(Path(args.yardstick).read_text())["feature_pass_ms"]
        res["yardstick"] = f"feature_pass_ms of {Path(args.yardstick).name}"
    res["yardstick_feature_pass_ms"] = yard
    res["contrib_pass_over_yardstick"] = res["contrib_pass_ms"] / yard
line = json.dumps(res)
print(line)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
