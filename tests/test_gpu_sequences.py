"""Call sequences on one handle against the CPU oracle (sequence_model.py).

Every stateful test elsewhere in the suite is a hand-written path that varies
one thing.  Here one handle goes through setter switches, size changes, camera
jumps, host and device frames of every output format, and the probes that
write into its buffers between frames; whatever came before, every frame must
equal the oracle's frame of (view, size, mode, cap) bit for bit, and
last_stats must say what the model predicts.

  a. directed sequences (sequence_model.DIRECTED): one row per transition
  b. seeded random sequences over the whole alphabet, with a bounded greedy
     shrink of a failing one
  c. the dilation radius of the depth cuts grows after a jump and decays again
  d. reach: what a, b and c together must have seen in last_stats
  e. an output tensor reused while the caller's stream still holds a reader
     of the previous frame (single handle pipelined; one-process group
     pipelined, whose gather runs on a stream of its own)

Device frames are read back only where the sequence synchronises anyway (host
frames, probes, the end), so pipelined stretches stay pipelined; each goes
into a tensor of its own or is cloned, guards included, on the caller's
stream.  An image or stats mismatch is reported with the sequence up to the
failing op and then shrunk by replaying on fresh handles; after a HIP error or
an unexpected GsError nothing is replayed."""
import copy
import re
import time
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import pytest

import sequence_model as M
from test_gpu_frame_shapes import Guarded

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

# d. filled from last_stats after synchronised frames by a, b and c
TALLY = {"front_only": 0, "front_only_open": 0, "dilate": 0, "dropped": 0, "default_binning": set(),
         "cut_after_mode": 0, "cut_after_cap": 0, "cut_after_size": 0}
RAN = set()
MAX_REPLAYS = 40


@pytest.fixture(scope="module", autouse=True)
def _report():
    from gaussian_splat_amd import _lib
    t = time.perf_counter()
    yield
    spent = sum(p.seconds for p in M.POOLS.values())
    print(f"\ntest_gpu_sequences ({_lib.LIB_PATH}): wall {time.perf_counter() - t:.1f} s, of which the oracle {spent:.1f} s")


@dataclass
class Fail:
    index: int   # op index
    what: str


class Stopped(Exception):
    """A HIP error or an unexpected GsError at op `index`: the handle is not used again."""

    def __init__(self, index, cause):
        super().__init__(f"op {index}: {type(cause).__name__}: {cause}")
        self.index = index


def _diff(got, want):
    """None when equal bit for bit, else (differing 32-bit words, first differing pixel (x, y))."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    H, W = got.shape[:2]
    ne = got.view(np.uint32).reshape(H, W, -1) != want.view(np.uint32).reshape(H, W, -1)
    if not ne.any():
        return None
    y, x = np.argwhere(ne.any(axis=-1))[0]
    return int(ne.sum()), (int(x), int(y))


def _handle(pool, **kw):
    from gaussian_splat_amd import InstancedSplatRenderer, Options
    r = InstancedSplatRenderer(pool.scene, Options(crop=False, sh_degree=pool.sh, **kw))
    r.initialize(0)
    return r


_LISTS = {}


def _whole_lists(pool, vi, si, mlab):
    """The bin lists of (view, size) as a fresh whole-list handle first gave them (MLAB: index order)."""
    key = (id(pool), vi, si, mlab)
    if key not in _LISTS:
        r = _handle(pool, depth_split=False, mode="mlab" if mlab else "tile")
        r.render_host(*pool.view(vi, si), *M.SIZES[si])
        _LISTS[key] = r.sorted_pairs()
        r.close()
    return _LISTS[key]


class Player:
    """Plays ops on one handle; compare() settles the device frames still pending."""

    def __init__(self, start, tally=None):
        self.pool = M.POOLS[start.get("pool", "sh0")]
        self.start, self.tally = start, tally
        self.model = M.Model(start["frames_in_flight"], start.get("si", 0))
        self.r = _handle(self.pool, binning=start["binning"], frames_in_flight=start["frames_in_flight"])
        self.pending = []     # (op index, what, getter, expected) of device frames not yet read back
        self.guards = {}
        self.switch = None    # "mode" / "cap" / "size": the op right before was that switch
        self.frame_switch = None  # ... before the last frame

    # ---- outputs
    def _guarded(self, W, H, words):
        """A reused guarded buffer, refilled with its sentinel on the caller's stream; words per pixel 4 or 1."""
        g = self.guards.get((W, H, words))
        if g is None:
            g = self.guards[(W, H, words)] = Guarded(W, H, bgra8=words == 1)
        else:
            g.buf.fill_(g.sent)
        return g

    @staticmethod
    def _snapshot(g):
        """The guarded buffer as it is at this point of the caller's stream; read (and its guards checked) later."""
        s = copy.copy(g)
        s.buf = g.buf.clone()
        return s.frame

    def _device_frame(self, kind, buf, V, P, W, H):
        import torch
        r = self.r
        if kind == "render_depth":
            if buf == "guarded":
                gc, gd = self._guarded(W, H, 4), self._guarded(W, H, 1)
                plane = gd.buf[gd.g:gd.g + gd.n].view(torch.float32).view(H, W)
                r.render_depth(V, P, W, H, out=gc.out, depth=plane)
                fc, fd = self._snapshot(gc), self._snapshot(gd)
                return lambda: (fc(), fd().view(np.float32).reshape(H, W))
            c, d = r.render_depth(V, P, W, H)
            return lambda: (c.cpu().numpy(), d.cpu().numpy())
        call = r.render if kind == "render" else r.render_bgra8
        if buf == "guarded":
            g = self._guarded(W, H, 4 if kind == "render" else 1)
            call(V, P, W, H, out=g.out)
            return self._snapshot(g)
        t = call(V, P, W, H)
        return lambda: t.cpu().numpy()

    def _expected(self, e):
        if e.kind in ("render", "render_host"):
            return self.pool.frame(e.vi, e.si, e.mode, e.cap)
        if e.kind in ("render_bgra8", "render_bgra8_host"):
            return self.pool.bgra8(e.vi, e.si, e.mode)
        depth, colour = self.pool.depth(e.vi, e.si, e.mode)
        assert _diff(colour, self.pool.frame(e.vi, e.si, e.mode, 0)) is None  # (one oracle, two entry points)
        return colour, depth

    @staticmethod
    def _judge(i, got, want):
        names = ("colour", "depth") if isinstance(want, tuple) else ("frame",)
        got, want = (got, want) if isinstance(want, tuple) else ((got,), (want,))
        for name, g, w in zip(names, got, want):
            d = _diff(g, w)
            if d:
                return Fail(i, f"{name} differs from the oracle in {d[0]} words, first at pixel {d[1]}")
        return None

    def compare(self):
        import torch
        torch.cuda.synchronize()
        pending, self.pending = self.pending, []
        for i, getter, want in pending:
            try:
                got = getter()
            except AssertionError as ex:  # (Guarded.frame: a guard word written, or a frame word never written)
                return Fail(i, f"guards: {ex}")
            f = self._judge(i, got, want)
            if f:
                return f
        return None

    # ---- stats
    def _stats(self, i):
        st = self.r.last_stats()
        bad = M.check_stats(st, self.model.last.stats(self.pool))
        if bad:
            return Fail(i, "last_stats: " + "; ".join(bad))
        t = self.tally
        if t is not None:
            if st["cut_frame"] and st["front_only"]:
                t["front_only"] += 1
                t["front_only_open"] += int(st["open_tiles"] > 0)
            if st["cut_frame"] and self.frame_switch:
                t["cut_after_" + self.frame_switch] += 1
            t["dilate"] += int(st["cut_dilate"] > 0)
            t["dropped"] += int(st["pairs_sorted"] < st["pairs"])
            if self.start["binning"] == "default":
                t["default_binning"].add(int(st["binning"]))
        return None

    # ---- one op
    def play(self, i, op):
        """None, or the first Fail this op brought to light."""
        from gaussian_splat_amd._lib import GsError
        m, r, pool = self.model, self.r, self.pool
        k, a = op.kind, op.arg
        switch, self.switch = self.switch, None
        if k in M.FRAME_OPS:
            e = m.step(op)
            self.frame_switch = switch
            W, H = M.SIZES[e.si]
            V, P = pool.view(e.vi, e.si)
            want = self._expected(e)
            if k in M.DEVICE_FRAMES:
                self.pending.append((i, self._device_frame(k, a, V, P, W, H), want))
                return None
            got = {"render_host": r.render_host, "render_bgra8_host": r.render_bgra8_host,
                   "render_depth_host": r.render_depth_host}[k](V, P, W, H)
            return self.compare() or self._judge(i, got, want) or self._stats(i)
        if k in M.SETTER_VALUES:
            m.step(op)
            getattr(r, k)(a)
            self.switch = {"set_mode": "mode", "set_cap": "cap"}.get(k)
            return None
        if k in M.CAMERA_OPS:
            m.step(op)
            self.switch = "size" if k == "size" else None
            return None
        m.step(op)
        if k == "last_stats":
            return self._stats(i) or self.compare()
        if k == "project_host":
            W, H = M.SIZES[m.si]
            rec, dk, nt = r.project_host(*pool.view(a, m.si), W, H)
            orec, odk, ont = pool.projection(a, m.si)
            vis = ont > 0
            if not (np.array_equal(nt, ont) and np.array_equal(dk[vis], odk[vis]) and
                    np.array_equal(rec[vis].view(np.uint32), orec[vis].view(np.uint32))):
                return Fail(i, "project_host differs from the oracle's projection")
            return self.compare()
        if k == "sorted_pairs":
            keys, vals = r.sorted_pairs()
            wk, wv = _whole_lists(pool, m.last.vi, m.last.si, m.last.mode == "mlab")
            if not (np.array_equal(keys, wk) and np.array_equal(vals, wv)):
                return Fail(i, f"sorted_pairs ({len(keys)} pairs) differ from a fresh whole-list handle's ({len(wk)})")
            return self.compare()
        assert k == "refused_depth"
        W, H = M.SIZES[m.si]
        try:
            (r.render_depth if a == "device" else r.render_depth_host)(*pool.view(m.vi, m.si), W, H)
        except GsError as ex:
            if ex.status != 7:
                raise
            return None
        return Fail(i, "render_depth under a cap or MLAB was not refused")

    def close(self):
        self.r.close()


def play(start, ops, tally=None):
    """Plays the sequence on a fresh handle: None, or the first Fail; Stopped after a HIP error or a GsError."""
    p = Player(start, tally)
    i = -1
    try:
        for i, op in enumerate(ops):
            f = p.play(i, op)
            if f:
                return f
        return p.compare()
    except Exception as ex:
        raise Stopped(i, ex) from ex
    finally:
        p.close()


def _lines(ops, upto=None):
    return "\n".join(f"{i:3d}  {op}" for i, op in enumerate(ops if upto is None else ops[:upto + 1]))


def shrink(start, ops, fail):
    """Bounded greedy shrink: cut the sequence after the failing op, then drop one op at a time, keeping
    each shorter sequence that is legal and still fails on a fresh handle; at most MAX_REPLAYS replays."""
    best, replays = list(ops), 0

    def fails(cand):
        nonlocal replays
        replays += 1
        return play(start, cand) is not None

    cut = list(ops[:fail.index + 1])
    if len(cut) < len(best) and fails(cut):
        best = cut
    j = len(best) - 2  # (the last op is the one that fails)
    while j >= 0 and replays < MAX_REPLAYS:
        cand = best[:j] + best[j + 1:]
        if M.legal_sequence(start, cand) and fails(cand):
            best = cand
        j -= 1
    return best, replays


def run_sequence(label, start, ops):
    try:
        f = play(start, ops, TALLY)
    except Stopped as ex:
        pytest.fail(f"{label} start {start}: stopped at {ex}\n(nothing replayed)\n{_lines(ops, ex.index)}")
    if f is None:
        return
    report = f"{label} start {start}: op {f.index} ({ops[f.index]}): {f.what}\n{_lines(ops, f.index)}"
    print(report)
    try:
        short, replays = shrink(start, ops, f)
    except Stopped as ex:
        pytest.fail(f"{report}\nshrink stopped at {ex}")
    pytest.fail(f"{report}\nshortest failing sequence found ({len(short)} ops, {replays} replays):\n{_lines(short)}")


# ------------------------------------------------------------- a. directed

@pytest.mark.parametrize("name,start,ops", M.DIRECTED, ids=[row[0] for row in M.DIRECTED])
def test_directed_sequence(built, name, start, ops):
    RAN.add("a")
    run_sequence(name, start, ops)


# --------------------------------------------------------------- b. random

@pytest.mark.parametrize("seed", M.SEEDS)
def test_random_sequence(built, seed):
    RAN.add("b")
    seq = M.generate(seed, M.LENGTH)
    run_sequence(f"seed {seed}", seq.start, seq.ops)


# ------------------------------------------------------------- c. dilation

def _cut_calm():
    """kCutCalm of renderer.cpp: calm frames per buffer set before the dilation radius drops by one."""
    src = (ROOT / "gaussian_splat_amd" / "csrc" / "host" / "renderer.cpp").read_text()
    m = re.search(r"constexpr int kCutCalm = (\d+);", src)
    assert m, "kCutCalm not found in renderer.cpp"
    return int(m.group(1))


@pytest.mark.parametrize("fif", [1, 2])
@pytest.mark.parametrize("binning", ["bin_first", "depth_first"])
def test_dilation_grows_and_decays(built, binning, fif):
    """far x3, near x3, far, then still at far.  A depth key is kDepthInf minus
    the half-float view depth, and the near view (distance 2) puts every splat
    ahead of the nearest one of the far view (distance 7): the jump in leaves
    no quadrant open (every pair lies ahead of the old cuts; measured: 0 open
    tiles in all four cases, printed below), the jump back out leaves every
    saturated bin's open (no pair lies ahead of the near view's cuts).  That
    jump is the one asserted: open_tiles > 0 on it, the set's cuts are then
    read dilated (cut_dilate > 0), and after kCutCalm calm frames per buffer
    set the radius is back at 0 and, bin-first, the frames emit their front
    pairs only again.  The radius climbs by one per frame that left quadrants
    open, to 3 at most, and each step down takes kCutCalm calm frames of the
    set, so 3 x kCutCalm x frames in flight still frames are the budget.  One
    frame in flight: host frames.  Two: device frames, synchronised one by
    one (a host frame never runs pipelined, and only pipelined frames
    alternate the two sets), so every frame's stats are settled either way."""
    import torch
    RAN.add("c")
    pool, si = M.POOLS["sh0"], 0
    W, H = M.SIZES[si]
    budget = 3 * _cut_calm() * fif
    r = _handle(pool, binning=binning, frames_in_flight=fif)
    model = M.Model(fif, si)
    log, grown, calm, decayed = [], False, 0, False
    path = [M.FAR] * 3 + [M.NEAR] * 3 + [M.FAR] * (1 + budget)
    jump = 6  # (the first frame back at far)
    for k, vi in enumerate(path):
        model.vi = vi
        e = model.step(M.Op("render_host") if fif == 1 else M.Op("render", "fresh"))
        V, P = pool.view(vi, si)
        if fif == 1:
            got = r.render_host(V, P, W, H)
        else:
            t = r.render(V, P, W, H)
            torch.cuda.synchronize()
            got = t.cpu().numpy()
        assert _diff(got, pool.frame(vi, si)) is None, (k, log)
        st = r.last_stats()
        assert not M.check_stats(st, e.stats(pool)), (k, M.check_stats(st, e.stats(pool)))
        log.append((st["open_tiles"], st["cut_dilate"], st["front_only"]))
        TALLY["dilate"] += int(st["cut_dilate"] > 0)
        if st["front_only"]:
            TALLY["front_only"] += 1
            TALLY["front_only_open"] += int(st["open_tiles"] > 0)
        if k == jump:
            assert st["open_tiles"] > 0, log
        if k > jump:
            grown = grown or st["cut_dilate"] > 0
            back = st["cut_dilate"] == 0 and (binning != "bin_first" or st["front_only"] == 1)
            calm = calm + 1 if grown and back else 0
            if calm >= fif:  # (every buffer set's last frame)
                decayed = True
                break
    r.close()
    print(f"{binning} fif {fif}: (open tiles, cut_dilate, front_only) per frame {log}")
    assert grown, log
    assert decayed, (budget, log)


# ---------------------------------------------------------------- d. reach

def test_reach():
    """What a, b and c together must have seen in last_stats after synchronised frames."""
    if RAN != {"a", "b", "c"}:
        pytest.skip("asserted over the directed, random and dilation tests together: run the whole module")
    print(TALLY)
    assert TALLY["front_only"] > 0                      # a front-only cut frame
    assert TALLY["front_only_open"] > 0                 # one that left quadrants open
    assert TALLY["dilate"] > 0                          # a frame that read dilated cuts
    assert TALLY["dropped"] > 0                         # a frame whose cuts dropped pairs (the cuts bite)
    assert TALLY["default_binning"] == {1, 2}, TALLY    # both orders picked by the binning-order model
    for sw in ("mode", "cap", "size"):                  # a cut frame directly after each switch
        assert TALLY["cut_after_" + sw] > 0, (sw, TALLY)


# ------------------------------------------------------- e. reused outputs

def _delay(call_ms):
    """Delay on the caller's stream: 20 x the measured call, between 5 and 100 ms, in _sleep cycles."""
    import torch
    torch.cuda._sleep(1000)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(10_000_000)
    e1.record()
    torch.cuda.synchronize()
    per_ms = 10_000_000 / e0.elapsed_time(e1)
    ms = min(max(20.0 * call_ms, 5.0), 100.0)
    return ms, int(ms * per_ms)


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _sleep_then_clone(out, call_ms):
    """The delay, then a reader of `out`, both on the caller's stream; returns the clone and the events around the delay."""
    import torch
    ms, cycles = _delay(call_ms)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(cycles)
    e1.record()
    return out.clone(), ms, (e0, e1)


def _caller(k):
    """The caller's stream: torch's default stream (k = 0) or the k-th of k new ones.  The runtime spreads a
    process's streams over a few hardware queues, and two streams that share a queue run in order whatever
    their events say: with four callers at least one does not share the gather stream's."""
    import contextlib

    import torch
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(k)]
    return torch.cuda.stream(streams[-1]) if k else contextlib.nullcontext()


@pytest.mark.parametrize("caller", [0, 1, 2, 3])
def test_reused_out_single_handle(built, caller):
    """Two frames in flight: frame B rendered into the tensor frame A is in,
    while the caller's stream still holds a delay and a clone of A.  The
    composite runs on the caller's stream, so the clone reads A."""
    with _caller(caller):
        _reused_out_single_handle()


def _reused_out_single_handle():
    import torch
    pool, si = M.POOLS["sh0"], 0
    W, H = M.SIZES[si]
    A, B = pool.view(0, si), pool.view(M.WIDE, si)
    r = _handle(pool, frames_in_flight=2)
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    scratch = torch.empty_like(out)
    for _ in range(3):
        r.render(*A, W, H, out=scratch)
    call_ms = _timed(lambda: r.render(*B, W, H, out=scratch))
    r.render(*A, W, H, out=out)
    kept, ms, (e0, e1) = _sleep_then_clone(out, call_ms)
    r.render(*B, W, H, out=out)
    torch.cuda.synchronize()
    print(f"single handle: call {call_ms:.3f} ms, delay asked {ms:.1f} ms, ran {e0.elapsed_time(e1):.1f} ms")
    assert e0.elapsed_time(e1) >= 0.8 * ms  # (the delay was one)
    assert _diff(kept.cpu().numpy(), pool.frame(0, si)) is None
    assert _diff(out.cpu().numpy(), pool.frame(M.WIDE, si)) is None
    r.close()


@pytest.mark.parametrize("caller", [0, 1, 2, 3])
def test_reused_out_group_pipelined(built, caller):
    """The one-process group, two ranks on one device over the copy
    transport, pipelined: rank 0's gather stream writes the caller's tensor,
    so it has to wait for what the caller's stream held when the call began
    (group.cpp pipelined_call, caller_ready).  Without that wait nothing
    orders the gather of frame B after the pending clone of frame A.
    Measured on an MI355X (delays of 10 to 17 ms, 20 x the call): the clone
    read A from all four caller streams with the wait and, on the build
    before it, without it too; this test pins the contract, it did not show
    the race there."""
    with _caller(caller):
        _reused_out_group_pipelined()


def _reused_out_group_pipelined():
    import torch

    from gaussian_splat_amd import ShardedGroup
    pool, si = M.POOLS["sh0"], 0
    W, H = M.SIZES[si]
    A, B = pool.view(0, si), pool.view(M.WIDE, si)
    one = _handle(pool)
    g = ShardedGroup(one, 2)
    g.initialize([0, 0], "copy")
    g.set_scheme("rows")
    g.set_frames_in_flight(2)
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    scratch = torch.empty_like(out)
    assert g.render_pipelined(*A, W, H, out=scratch) is None
    assert g.flush(W, H, out=scratch) is not None

    def call():
        assert g.render_pipelined(*B, W, H, out=scratch) is None
        assert g.flush(W, H, out=scratch) is not None

    call_ms = _timed(call)
    assert g.render_pipelined(*A, W, H, out=out) is None
    assert g.flush(W, H, out=out) is not None
    kept, ms, (e0, e1) = _sleep_then_clone(out, call_ms)
    assert g.render_pipelined(*B, W, H, out=out) is None
    assert g.flush(W, H, out=out) is not None
    torch.cuda.synchronize()
    print(f"group: call {call_ms:.3f} ms, delay asked {ms:.1f} ms, ran {e0.elapsed_time(e1):.1f} ms")
    assert e0.elapsed_time(e1) >= 0.8 * ms
    d_kept, d_out = _diff(kept.cpu().numpy(), pool.frame(0, si)), _diff(out.cpu().numpy(), pool.frame(M.WIDE, si))
    g.close()
    one.close()
    assert d_kept is None, f"the clone of frame A differs from A's oracle frame: {d_kept}"
    assert d_out is None, d_out
