"""Call sequences on one gs_handle: the pool of frames, the op alphabet, the
model and the generator (plain helper of test_gpu_sequences.py and
test_sequence_model.py; imports and generates without a GPU).

A handle carries state from frame to frame (renderer.cpp: the depth cuts'
tables per buffer set, the dilation controller, the binning-order model, the
pair buffers' capacity, the two sets of a pipelined handle, the open
quadrants' saved states, the kernel-event ring), and five setters only write
h->opt and leave the next frame to sort out the rest.  Whatever the history,
every frame must be the oracle's, bit for bit.  This module says what a
sequence of calls is and what each call must give; test_gpu_sequences.py
plays sequences on a handle.

The pool.  One scene (the 100,000 splats of test_depth_mixed_and_pipelined's,
SH 0, scale x3) and an SH3 scene of 40,000 splats for one directed sequence;
two frame sizes, 1037 x 531 (561 bins: strip composite, ragged right and
bottom) and 333 x 211 (77 bins: one workgroup per tile); six views per size.
Expected frames come from the CPU oracle only (O.render, O.to_bgra8 of it,
depth_ref), computed on first use and kept per (view, size, mode, cap).

Ops.  One op per step:
  frames   render[guarded|fresh], render_host, render_bgra8[guarded|fresh],
           render_bgra8_host, render_depth[guarded|fresh], render_depth_host
           (guarded: a reused device buffer between NaN-sentinel guards,
           cloned on the caller's stream; fresh: a new tensor per frame)
  camera   orbit (the next of the three orbit steps), jump(view), size (the
           other frame size); "same view" is the absence of a camera op, and
           the generator's weights make that the usual case between frames
  setters  set_mode, set_cap, set_depth_split, set_frames_in_flight,
           set_stage_timing
  probes   last_stats, project_host(view), sorted_pairs,
           refused_depth[device|host] (render_depth under a cap or MLAB:
           GS_ERR_UNSUPPORTED, and the next frame must still be right)

Legality (Model.legal).  BGRA8 and depth frames in tile / live50 without a cap
only; refused_depth only outside that; sorted_pairs only after a frame the
model knows had whole lists (depth_split off, a cap, or MLAB) with no
project_host since (it rewrites the set's projection buffers); MLAB and a cap
never together (gs_render refuses that combination halfway through a frame,
which is not part of this alphabet); a setter changes its value.

The model does not predict front_only, cut_dilate or binning: they depend on
when the device's counts reach the host, and the image must not."""
from __future__ import annotations

import functools
import time
from dataclasses import dataclass

import numpy as np

SIZES = ((1037, 531), (333, 211))
VIEWS = ("default", "orbit1", "orbit2", "far", "near", "wide")
ORBIT = (0, 1, 2)  # view indices of the orbit steps
FAR, NEAR, WIDE = 3, 4, 5
MODES = ("tile", "live50", "mlab")
CAPS = (0, 32, 50)
BINNINGS = ("default", "depth_first", "bin_first")
BUFFERS = ("guarded", "fresh")

DEVICE_FRAMES = ("render", "render_bgra8", "render_depth")
HOST_FRAMES = ("render_host", "render_bgra8_host", "render_depth_host")
FRAME_OPS = ("render", "render_host", "render_bgra8", "render_bgra8_host", "render_depth", "render_depth_host")
CAMERA_OPS = ("orbit", "jump", "size")
SETTER_VALUES = {"set_mode": MODES, "set_cap": CAPS, "set_depth_split": (False, True),
                 "set_frames_in_flight": (1, 2), "set_stage_timing": (0, 1, 2)}
SETTER_OPS = tuple(SETTER_VALUES)
PROBE_OPS = ("last_stats", "project_host", "sorted_pairs", "refused_depth")

SAT_ALPHA = 0.99      # a pixel the composite stopped at (both rules break at T = 0.01)
SAT_MIN_SHARE = 0.15  # of a frame's pixels: below that the depth cuts do not bite
# A bin's list is cut only where every quadrant of the bin finished, so the same share is asked of the
# 32 x 32 bins saturated in all their pixels.  At scale x2 the pixel share holds (0.28 .. 0.72) but no bin
# of the default and far views saturates whole, and no list was ever cut (pairs_sorted == pairs on every
# still frame on an MI355X); at x3 the oracle gives 211 .. 513 of 561 and 23 .. 70 of 77 bins.
SCENE_SCALE = 3.0


def camera(vi, W, H):
    """(view, projection) of pool view `vi` at W x H, from the reference's default camera."""
    from gaussian_splat_amd.api import default_camera
    cam = default_camera(W, H)
    name = VIEWS[vi]
    if name.startswith("orbit"):
        k = int(name[5:])
        cam.orbit(0.02 * k, 0.005 * k)
    elif name == "far":
        cam.setDistance(7.0)
    elif name == "near":  # (the recipe of test_depth_cuts_jump_opens_tiles: its cuts lie ahead of every far key)
        cam.setDistance(2.0)
        cam.orbit(0.4, 0.1)
    elif name == "wide":
        cam.setDistance(3.5)
        cam.orbit(2.2, 0.3)
    return cam.getViewMatrix(), cam.getProjectionMatrix()


class Pool:
    """A scene, its views and the oracle's frames of them, computed on first
    use, kept and never changed.  `seconds`: oracle time spent so far."""

    def __init__(self, n, sh, scale):
        self.n, self.sh, self.scale = n, sh, scale
        self.seconds = 0.0
        self._frames, self._stats, self._proj, self._zf, self._depth = {}, {}, {}, {}, {}

    @functools.cached_property
    def scene(self):
        from gaussian_splat_amd import scene as S
        W, H = SIZES[0]
        sc = S.activate(S.synthetic_raw(self.n, seed=9, aspect=W / H, rest=self.sh > 0), self.sh)
        sc.scale *= np.float32(self.scale)
        return sc

    @functools.lru_cache(maxsize=None)
    def view(self, vi, si):
        return camera(vi, *SIZES[si])

    def _timed(self, fn, *a, **kw):
        t = time.perf_counter()
        out = fn(*a, **kw)
        self.seconds += time.perf_counter() - t
        return out

    def frame(self, vi, si, mode="tile", cap=0):
        """The oracle's fp32 RGBA frame."""
        key = (vi, si, mode, cap)
        if key not in self._frames:
            from oracle import oracle_py as O
            W, H = SIZES[si]
            ref, st = self._timed(O.render, self.scene, *self.view(vi, si), W, H, sh_degree=self.sh, mode=mode, cap=cap)
            ref.setflags(write=False)
            self._frames[key] = ref
            self._stats.setdefault((vi, si), st)
        return self._frames[key]

    def oracle_stats(self, vi, si):
        """OraStats of the view (visible splats, 16 x 16 tile pairs): the same for every rule."""
        if (vi, si) not in self._stats:
            self.frame(vi, si)
        return self._stats[(vi, si)]

    def bgra8(self, vi, si, mode="tile"):
        key = (vi, si, mode, "bgra8")
        if key not in self._frames:
            from oracle import oracle_py as O
            want = self._timed(O.to_bgra8, self.frame(vi, si, mode, 0))
            want.setflags(write=False)
            self._frames[key] = want
        return self._frames[key]

    def depth(self, vi, si, mode="tile"):
        """(depth image, colour frame) of depth_ref: one projection per view, shared by the rules."""
        key = (vi, si, mode)
        if key not in self._depth:
            import depth_ref
            W, H = SIZES[si]
            V, P = self.view(vi, si)
            if (vi, si) not in self._zf:
                self._zf[(vi, si)] = self._timed(depth_ref.project_zf, self.scene, V, P, W, H, self.sh)
            self._depth[key] = self._timed(depth_ref.depth_from_projection, self.scene, V, P, W, H, mode, self.sh,
                                           self._zf[(vi, si)])
        return self._depth[key]

    def projection(self, vi, si):
        """(records, depth keys, tiles per splat) of O.project."""
        if (vi, si) not in self._proj:
            from oracle import oracle_py as O
            W, H = SIZES[si]
            self._proj[(vi, si)] = self._timed(O.project, self.scene, *self.view(vi, si), W, H, self.sh)
        return self._proj[(vi, si)]


POOLS = {"sh0": Pool(100000, 0, SCENE_SCALE), "sh3": Pool(40000, 3, 4.0)}


@dataclass(frozen=True)
class Op:
    kind: str
    arg: object = None

    def __str__(self):
        if self.kind in DEVICE_FRAMES or self.kind == "refused_depth":
            return f"{self.kind}[{self.arg}]"
        if self.kind in ("jump", "project_host"):
            return f"{self.kind}({VIEWS[self.arg]})"
        return self.kind if self.arg is None else f"{self.kind}({self.arg})"


@dataclass(frozen=True)
class Expect:
    """What a frame op must give: the oracle's frame of (view, size, mode, cap)."""
    kind: str
    vi: int
    si: int
    mode: str
    cap: int
    cut_frame: bool
    cuts: bool = True  # the frame's buffer set may hold cuts (False: it cannot, see Model.step)

    def stats(self, pool):
        """The fields of last_stats the model predicts after this frame, synchronised."""
        W, H = SIZES[self.si]
        want = {"width": W, "height": H, "visible": int(pool.oracle_stats(self.vi, self.si)["visible"]),
                "cut_frame": int(self.cut_frame)}
        if not self.cuts:  # whole lists, whatever the timing: nothing cut, nothing left open, nothing dilated
            want.update(open_tiles=0, front_only=0, cut_dilate=0)
        return want


def check_stats(st, want):
    """Mismatches of a last_stats dict against Expect.stats(), as a list of strings (empty: none)."""
    bad = [f"{k}: {st[k]} != {v}" for k, v in want.items() if st[k] != v]
    if not st["pairs_sorted"] <= st["pairs"]:
        bad.append(f"pairs_sorted {st['pairs_sorted']} > pairs {st['pairs']}")
    if want.get("front_only") == 0 and st["pairs_sorted"] != st["pairs"]:  # (Expect.cuts is False)
        bad.append(f"pairs_sorted {st['pairs_sorted']} != pairs {st['pairs']} on a frame that can have no cuts")
    if not 0 <= st["open_tiles"] <= 16 * st["tiles"]:  # (8 x 8 quadrants of the 32 x 32 bins)
        bad.append(f"open_tiles {st['open_tiles']} outside 0..{16 * st['tiles']}")
    return bad


class Model:
    """The options and the view of a handle under a sequence of ops."""

    def __init__(self, frames_in_flight=1, si=0, vi=0):
        self.mode, self.cap, self.depth_split, self.stage_timing = "tile", 0, True, 0
        self.frames_in_flight = frames_in_flight
        self.si, self.vi = si, vi
        self.last = None        # Expect of the last frame
        self.pairs_ok = False   # sorted_pairs may be asked: the last frame had whole lists, nothing rewrote the set
        # Which frames cannot have cuts (renderer.cpp setup_cuts): a buffer set holds cuts only from a
        # depth-cut frame on that set at this frame size and composite rule.  A frame runs pipelined, on the
        # other set, when two frames are in flight, its output is a device buffer and stage_timing is not 1.
        self.set, self.valid, self.cut_key = 0, [False, False], None

    def _plain(self):
        return self.mode in ("tile", "live50") and self.cap == 0

    def cut_frame(self):
        return self.depth_split and self._plain()

    def legal(self, op):
        k, a = op.kind, op.arg
        if k in ("render", "render_host"):
            return a in BUFFERS if k == "render" else a is None
        if k in FRAME_OPS:
            return self._plain() and (a in BUFFERS if k in DEVICE_FRAMES else a is None)
        if k == "orbit":
            return self.vi in ORBIT
        if k == "jump":
            return a in range(len(VIEWS)) and a != self.vi
        if k == "size":
            return True
        if k in SETTER_VALUES:
            if a not in SETTER_VALUES[k] or a == getattr(self, k[4:]):
                return False
            if k == "set_mode" and a == "mlab":
                return self.cap == 0
            if k == "set_cap" and a > 0:
                return self.mode != "mlab"
            return True
        if k == "last_stats":
            return self.last is not None
        if k == "project_host":
            return a in range(len(VIEWS))
        if k == "sorted_pairs":
            return self.pairs_ok
        if k == "refused_depth":
            return a in ("device", "host") and not self._plain()
        return False

    def step(self, op):
        """Apply a legal op; a frame op returns its Expect."""
        assert self.legal(op), f"illegal op {op}"
        k, a = op.kind, op.arg
        if k in FRAME_OPS:
            if self.frames_in_flight == 2 and k in DEVICE_FRAMES and self.stage_timing != 1:
                self.set ^= 1
            if self.cut_key != (self.si, self.mode):
                self.valid, self.cut_key = [False, False], (self.si, self.mode)
            cuts = self.cut_frame() and self.valid[self.set]
            self.valid[self.set] = self.cut_frame()
            self.last = Expect(k, self.vi, self.si, self.mode, self.cap, self.cut_frame(), cuts)
            self.pairs_ok = not self.last.cut_frame
            return self.last
        if k == "orbit":
            self.vi = ORBIT[(ORBIT.index(self.vi) + 1) % len(ORBIT)]
        elif k == "jump":
            self.vi = a
        elif k == "size":
            self.si ^= 1
        elif k in SETTER_VALUES:
            setattr(self, k[4:], a)
        elif k == "project_host":
            self.pairs_ok = False
        return None


def legal_sequence(start, ops):
    m = Model(start["frames_in_flight"], start.get("si", 0), start.get("vi", 0))
    for op in ops:
        if not m.legal(op):
            return False
        m.step(op)
    return True


# ---------------------------------------------------------------- generator

# Frame ops weigh most and camera ops little, so runs of frames at one view
# are the usual case: cuts act only after two or three still frames on a
# buffer set.  The op after a setter is always a frame: the transition is what
# the sequence is for.
GROUP_WEIGHTS = {"frame": 0.56, "camera": 0.12, "setter": 0.20, "probe": 0.12}
CAMERA_WEIGHTS = {"orbit": 0.35, "jump": 0.40, "size": 0.25}


def _candidates(group):
    if group == "frame":
        return {k: [Op(k, b) for b in BUFFERS] if k in DEVICE_FRAMES else [Op(k)] for k in FRAME_OPS}
    if group == "camera":
        return {"orbit": [Op("orbit")], "jump": [Op("jump", v) for v in range(len(VIEWS))], "size": [Op("size")]}
    if group == "setter":
        return {k: [Op(k, v) for v in vals] for k, vals in SETTER_VALUES.items()}
    return {"last_stats": [Op("last_stats")], "project_host": [Op("project_host", v) for v in range(len(VIEWS))],
            "sorted_pairs": [Op("sorted_pairs")], "refused_depth": [Op("refused_depth", a) for a in ("device", "host")]}


@dataclass(frozen=True)
class Sequence:
    seed: int
    start: dict   # Options of the handle: binning, frames_in_flight
    ops: tuple

    def lines(self, upto=None):
        """One line per op, through op index `upto`."""
        ops = self.ops if upto is None else self.ops[:upto + 1]
        return [f"{i:3d}  {op}" for i, op in enumerate(ops)]

    def __str__(self):
        return "\n".join([f"seed {self.seed} start {self.start}"] + self.lines())


def generate(seed, length=40):
    """The sequence of (seed, length): start options and ops, all drawn from numpy's default_rng(seed)."""
    rng = np.random.default_rng(seed)
    start = {"binning": BINNINGS[int(rng.integers(len(BINNINGS)))], "frames_in_flight": int(rng.integers(1, 3))}
    m = Model(start["frames_in_flight"])
    groups, gw = list(GROUP_WEIGHTS), np.array(list(GROUP_WEIGHTS.values()))
    ops, after_setter = [], False
    while len(ops) < length:
        group = "frame" if after_setter or not ops else groups[int(rng.choice(len(groups), p=gw / gw.sum()))]
        kinds = {k: [o for o in v if m.legal(o)] for k, v in _candidates(group).items()}
        kinds = {k: v for k, v in kinds.items() if v}
        if not kinds:
            continue
        names = list(kinds)
        if group == "camera":
            w = np.array([CAMERA_WEIGHTS[k] for k in names])
            kind = names[int(rng.choice(len(names), p=w / w.sum()))]
        else:
            kind = names[int(rng.integers(len(names)))]
        op = kinds[kind][int(rng.integers(len(kinds[kind])))]
        m.step(op)
        ops.append(op)
        after_setter = group == "setter"
    return Sequence(seed, start, tuple(ops))


# (chosen, among the first 400, so that together they cover the alphabet: test_sequence_model.py)
SEEDS = (1, 6, 41, 83, 119, 145, 172, 203)
LENGTH = 40


# ---------------------------------------------------------- directed table

def _still(n, kind="render", buf="fresh"):
    return [Op(kind, buf if kind in DEVICE_FRAMES else None)] * n


R, RG, RH = Op("render", "fresh"), Op("render", "guarded"), Op("render_host")
B8, D, ST = Op("render_bgra8", "fresh"), Op("render_depth", "fresh"), Op("last_stats")


def _row(name, ops, fif=1, binning="default", si=0, pool="sh0"):
    return name, {"binning": binning, "frames_in_flight": fif, "si": si, "pool": pool}, tuple(ops)


def _both(name, ops, **kw):
    return [_row(f"{name}-fif{f}", ops, fif=f, **kw) for f in (1, 2)]


# name, start, ops: each row pins the transition its name says
DIRECTED = [
    # a rule switch drops the cuts of both sets; the frame after each switch is a cut frame without cuts
    *_both("mode_tile_live50_tile",
           [R, ST] + _still(2) + [Op("set_mode", "live50"), R, ST] + _still(2, buf="guarded") +
           [Op("set_mode", "tile"), RH, R, RG]),
    # one capped frame between cut frames: it invalidates its own set's cuts only, with two frames in
    # flight the other set still holds older ones
    *_both("cap_one_frame", _still(3) + [Op("set_cap", 32), R, Op("set_cap", 0), R, ST, R, RG, RH]),
    *_both("cap_one_frame_bin_first", _still(3) + [Op("set_cap", 32), R, Op("set_cap", 0), R, ST, R, RG, RH],
           binning="bin_first"),
    # one whole-list frame (its lists read back), then cuts again, the near jump, and the jump back out,
    # which opens quadrants (the far view's depth keys all lie behind the near view's cuts)
    *_both("split_off_one_frame",
           _still(3) + [Op("set_depth_split", False), R, Op("sorted_pairs"), Op("set_depth_split", True),
                        Op("jump", NEAR), R, ST, R, R, Op("jump", FAR), R, ST, R, RH]),
    # two MLAB frames (index-order lists, no cuts) and back
    *_both("mlab_two_frames", _still(3) + [Op("set_mode", "mlab"), R, RG, Op("set_mode", "tile"), R, ST, R, RH]),
    # out of pipelining and back in the middle of an orbit; a host frame and a BGRA8 frame inside the pipelined stretch
    _row("fif_2_1_2_mid_orbit",
         [R, Op("orbit"), R, RG, Op("orbit"), RH, R, B8, Op("set_frames_in_flight", 1), Op("orbit"), R, R,
          Op("set_frames_in_flight", 2), Op("orbit"), R, RG, Op("orbit"), R, RH], fif=2),
    # stage_timing 2 turns the aux totals stream off (timing events in the preprocess's dispatch), 1 turns
    # pipelining off: across cut frames, front-only ones included
    *[_row(f"stage_timing_0_2_1_0-{b}",
           _still(3) + [Op("set_stage_timing", 2), R, R, ST, Op("set_stage_timing", 1), R, R, ST,
                        Op("set_stage_timing", 0), R, R, RH], fif=2, binning=b) for b in ("default", "bin_first")],
    # project_host of another view rewrites the current set's records, depth keys and rects between cut frames
    *_both("project_host_between_cut_frames", _still(3) + [Op("project_host", WIDE), R, ST, R, RH], binning="bin_first"),
    # a refused render_depth changes nothing: the next cut frame, a depth frame, is right
    *_both("refused_depth_then_depth",
           _still(3) + [Op("set_cap", 32), Op("refused_depth", "device"), Op("set_cap", 0), D, ST, R, D, RH]),
    # small frame to large: the pair buffers grow and the cut tables are regrown; back, the near jump and out again
    *_both("size_up_and_down",
           _still(3) + [Op("size"), R, ST, R, R, Op("size"), R, ST, Op("jump", NEAR), R, ST, R, R,
                        Op("jump", FAR), R, ST, R, RH], si=1),
    # SH3: depth and BGRA8 frames alternating along an orbit, two frames in flight
    _row("sh3_depth_bgra8_orbit",
         [D, Op("orbit"), B8, Op("orbit"), D, Op("orbit"), B8, D, Op("orbit"), B8, Op("orbit"), D, B8, ST, RH],
         fif=2, pool="sh3"),
]
