"""bench.py on one GPU, small: a plain run times its frames and prints the
headline line without the probes; --full adds them and times the same frames;
--dump-outputs writes the last timed frame, the same from both and within the
north star's 1e-4 of the CPU oracle's frame of the same scene and camera."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import NORTH_STAR_TOL

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
N, W, H, SH, SEED = 20000, 256, 192, 3, 2  # (the default config's seed and SH degree, a small scene and frame)
SIZE = ["--splats", str(N), "--width", str(W), "--height", str(H)]
PROBES = ("roofline", "cpu_baseline", "cpu_baseline_1core")


def _bench(args, out):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", *SIZE, "--dump-outputs", str(out), *args]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=str(ROOT))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), np.load(out / "frame.npy")


@pytest.fixture(scope="module")
def plain(built, tmp_path_factory):
    return _bench(["--steps", "3", "--warmup", "1"], tmp_path_factory.mktemp("plain"))


def test_plain_run_is_the_headline_alone(plain):
    d, frame = plain
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["config"]["global_splats"] == N
    assert d["unit"] == "Msplats/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and abs(d["value"] - N / (d["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * d["value"]
    assert d["settled"] is None and d["orbit"] is None and d["stages"] == {} and d["standalone_kernel_ms"] == {}
    assert not any(k in d for k in PROBES)
    assert frame.dtype == np.float32 and frame.shape == (H, W, 4)


def test_dumped_frame_matches_oracle(plain):
    from gaussian_splat_amd import scene as S
    from gaussian_splat_amd.api import default_camera
    from oracle import oracle_py as O
    sc = S.activate(S.synthetic_raw(N, seed=SEED, aspect=W / H, rest=True), SH)
    cam = default_camera(W, H)
    ref, _ = O.render(sc, cam.getViewMatrix(), cam.getProjectionMatrix(), W, H, sh_degree=SH)
    assert ref[..., 3].max() > 0.5
    assert float(np.abs(plain[1] - ref).max()) <= NORTH_STAR_TOL


def test_full_run_adds_the_probes_to_the_same_frames(plain, tmp_path):
    d, frame = _bench(["--full", "--steps", "3", "--warmup", "1", "--settled-probe", "2", "--cpu-seconds", "0.1",
                       "--pmc", "0"], tmp_path)
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert d["settled"]["extra_frames"] == 2 and d["settled"]["ms_per_step"] > 0 and d["orbit"]["ms_per_step"] > 0
    assert set(d["standalone_kernel_ms"]) == {"preprocess", "composite"} and "composite" in d["stages"]
    assert all(k in d for k in PROBES) and d["hbm_gbs"] > 0
    np.testing.assert_array_equal(frame.view(np.uint32), plain[1].view(np.uint32))
