"""The sequence generator and the pool of test_gpu_sequences.py, checked
without a GPU: the generator is deterministic and emits only legal sequences,
the committed seeds cover the alphabet, and the pool's oracle frames are such
that depth cuts bite and the pair buffers have to grow."""
import numpy as np
import pytest

import sequence_model as M


@pytest.fixture(scope="module")
def sequences():
    return [M.generate(s, M.LENGTH) for s in M.SEEDS]


def test_generator_is_deterministic(sequences):
    for s, seq in zip(M.SEEDS, sequences):
        again = M.generate(s, M.LENGTH)
        assert again == seq and str(again) == str(seq)
        assert len(seq.ops) == M.LENGTH
        assert seq.lines(3) == str(seq).split("\n")[1:5]  # one line per op
    assert len({seq.ops for seq in sequences}) == len(M.SEEDS)


def _replay(start, ops):
    """Every op legal when it comes; no sorted_pairs after a possibly cut frame, no BGRA8 (or depth frame)
    outside tile / live50 without a cap -- checked here on their own, beside Model.legal."""
    m = M.Model(start["frames_in_flight"], start.get("si", 0))
    cut_possible = True
    for i, op in enumerate(ops):
        assert m.legal(op), (i, str(op))
        if op.kind in ("render_bgra8", "render_bgra8_host", "render_depth", "render_depth_host"):
            assert m.mode in ("tile", "live50") and m.cap == 0, (i, str(op))
        if op.kind == "sorted_pairs":
            assert not cut_possible, (i, str(op))
        if op.kind == "refused_depth":
            assert m.cap > 0 or m.mode == "mlab", (i, str(op))
        assert not (m.mode == "mlab" and m.cap > 0)
        e = m.step(op)
        if op.kind in M.FRAME_OPS:
            assert e is not None and (e.vi, e.si, e.mode, e.cap) == (m.vi, m.si, m.mode, m.cap)
            cut_possible = m.depth_split and m.cap == 0 and m.mode in ("tile", "live50")
            assert e.cut_frame == cut_possible
        elif op.kind == "project_host":
            cut_possible = True  # (not a cut, but the set's buffers are rewritten: no sorted_pairs either)
        else:
            assert e is None


def test_every_sequence_is_legal(sequences):
    for seq in sequences:
        _replay(seq.start, seq.ops)
    for seed in range(100, 300):  # and whatever else it can emit
        seq = M.generate(seed, 30)
        _replay(seq.start, seq.ops)
        assert seq.start["binning"] in M.BINNINGS and seq.start["frames_in_flight"] in (1, 2)
    for name, start, ops in M.DIRECTED:
        _replay(start, ops)
    assert len({name for name, _, _ in M.DIRECTED}) == len(M.DIRECTED)


def test_committed_seeds_cover_the_alphabet(sequences):
    ops = [op for seq in sequences for op in seq.ops]
    for k, vals in M.SETTER_VALUES.items():
        for v in vals:
            assert M.Op(k, v) in ops, (k, v)
    seen = {op.kind for op in ops}
    for k in M.FRAME_OPS + M.CAMERA_OPS + M.PROBE_OPS:
        assert k in seen, k
    for k in M.DEVICE_FRAMES:
        for b in M.BUFFERS:
            assert M.Op(k, b) in ops, (k, b)
    # every setter kind directly followed by every frame op kind
    pairs = {(a.kind, b.kind) for seq in sequences for a, b in zip(seq.ops, seq.ops[1:])}
    missing = [(s, f) for s in M.SETTER_OPS for f in M.FRAME_OPS if (s, f) not in pairs]
    assert not missing, missing
    assert {seq.start["binning"] for seq in sequences} == set(M.BINNINGS)
    assert {seq.start["frames_in_flight"] for seq in sequences} == {1, 2}


def _whole_bins(frame):
    """Share of the 32 x 32 bins whose pixels (those inside the frame) are all saturated."""
    sat = frame[..., 3] >= M.SAT_ALPHA
    H, W = sat.shape
    bins = [sat[y:y + 32, x:x + 32].all() for y in range(0, H, 32) for x in range(0, W, 32)]
    return float(np.mean(bins))


def test_pool_conditions(built):
    """The oracle's frames of the pool: at the default, near and far views, in
    tile and live50 without a cap, at least 15 % of the pixels are saturated
    (A >= 0.99; below that share the cuts do not bite) and so are all the
    pixels of at least 15 % of the bins (a list is cut only where its whole
    bin finished), and the largest pair
    count of the pool is at least twice the smallest (the size change supplies
    it), so a handle that walks the pool has to grow its pair buffers."""
    pool = M.POOLS["sh0"]
    for si in range(len(M.SIZES)):
        for vi in (M.VIEWS.index("default"), M.NEAR, M.FAR):
            for mode in ("tile", "live50"):
                share = float((pool.frame(vi, si, mode, 0)[..., 3] >= M.SAT_ALPHA).mean())
                print(f"{M.SIZES[si]} {M.VIEWS[vi]} {mode}: saturated {share:.3f}")
                assert share >= M.SAT_MIN_SHARE, (M.SIZES[si], M.VIEWS[vi], mode, share)
                bins = _whole_bins(pool.frame(vi, si, mode, 0))
                print(f"{M.SIZES[si]} {M.VIEWS[vi]} {mode}: bins saturated whole {bins:.3f}")
                assert bins >= M.SAT_MIN_SHARE, (M.SIZES[si], M.VIEWS[vi], mode, bins)
    pairs = [int(pool.oracle_stats(vi, si)["pairs"]) for si in range(len(M.SIZES)) for vi in range(len(M.VIEWS))]
    print(f"oracle pairs {min(pairs)}..{max(pairs)}")
    assert min(pairs) > 0 and max(pairs) >= 2 * min(pairs), pairs
    # the views are six different ones at each size
    for si in range(len(M.SIZES)):
        mats = {np.asarray(pool.view(vi, si)[0], np.float32).tobytes() for vi in range(len(M.VIEWS))}
        assert len(mats) == len(M.VIEWS)
