"""The multi-GPU headline rule of bench.py (README): `value` is
the rows scheme's whenever rows is at least as fast as bands at that world
size; otherwise it is bands', named as the replicated scheme."""
import importlib.util
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("gs_bench", ROOT / "bench.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)  # (defines the functions; main runs only as a script)
    return m


def test_rows_headline_when_at_least_as_fast():
    b = _bench()
    assert b.headline({"rows": {"ms": 0.30}, "bands": {"ms": 0.42}}, ["bands", "rows"]) == ("rows", ["rows", "bands"])
    assert b.headline({"rows": {"ms": 0.42}, "bands": {"ms": 0.42}}, ["bands", "rows"])[0] == "rows"  # (ties: rows)


def test_bands_headline_only_when_faster_and_named_replicated():
    b = _bench()
    head, exact = b.headline({"rows": {"ms": 1.4}, "bands": {"ms": 0.61}}, ["bands", "rows"])
    assert head == "bands" and exact == ["rows", "bands"]
    text = b.scheme_choice(head, exact, 2)
    assert text.startswith("bands:") and "replicated" in text and "world size 2" in text


def test_single_scheme_runs():
    b = _bench()
    assert b.headline({"rows": {"ms": 1.0}}, ["rows"]) == ("rows", ["rows"])
    assert b.headline({"bands": {"ms": 1.0}}, ["bands"]) == ("bands", ["bands"])
    assert b.headline({}, ["slabs"]) == ("slabs", [])
    assert b.scheme_choice("rows", ["rows"], 8) == "rows"


def test_plain_run_leaves_the_probes_out(monkeypatch):
    """Without --full the options of the probes are off whatever they say;
    with it they hold as given."""
    b = _bench()
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "3", "--pmc", "1", "--settled-probe", "7"])
    a = b.parse()
    assert not a.full and a.steps == 3
    assert (a.settled_probe, a.orbit_probe, a.cpu_baseline, a.pmc, a.no_stage_timing) == (0, 0, 0, 0, True)
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--settled-probe", "7", "--cpu-baseline", "0"])
    a = b.parse()
    assert a.full and (a.settled_probe, a.orbit_probe, a.cpu_baseline, a.pmc, a.no_stage_timing) == (7, 1, 0, 1, False)


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: a frame within DUMP_LIMIT is written whole; a larger one
    as the same seeded sample of its pixels on every call, with their indices."""
    import numpy as np
    b = _bench()
    frame = np.random.default_rng(3).random((37, 53, 4), dtype=np.float32)
    b.dump_outputs(tmp_path / "whole", frame)
    got = np.load(tmp_path / "whole" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, frame)
    assert not (tmp_path / "whole" / "frame_pixels.npy").exists()
    monkeypatch.setattr(b, "DUMP_LIMIT", (16 + 8) * 100)  # room for 100 RGBA pixels and their indices
    for d in ("s1", "s2"):
        b.dump_outputs(tmp_path / d, frame)
    px, idx = np.load(tmp_path / "s1" / "frame.npy"), np.load(tmp_path / "s1" / "frame_pixels.npy")
    assert px.dtype == np.float32 and px.shape == (100, 4) and idx.dtype == np.float64 and idx.shape == (100,)
    assert px.nbytes + idx.nbytes <= (16 + 8) * 100 and len(set(idx.tolist())) == 100 and (np.diff(idx) > 0).all()
    assert np.array_equal(px, frame.reshape(-1, 4)[idx.astype(np.int64)])
    assert np.array_equal(px, np.load(tmp_path / "s2" / "frame.npy"))
    assert np.array_equal(idx, np.load(tmp_path / "s2" / "frame_pixels.npy"))
