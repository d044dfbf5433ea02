"""A plain `bench.py` run (no --full) as the driver launches it: the headline line only, `--steps` timed steps, and `--dump-outputs`
writing the last timed step's outputs -- identical from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--gaussians", "16384", "--views", "8"]


def _bench(extra, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_line_and_dumped_outputs(gpu_device, tmp_path):
    dumps = [tmp_path / "a", tmp_path / "b"]
    lines = [_bench(["--dump-outputs", str(d)]) for d in dumps]
    for d in lines:
        assert d["metric"].startswith("rendered views/sec") and d["unit"] == "views/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f32" and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0
        assert abs(d["value"] - 8 * 3 / (d["ms_per_step"] * 3e-3)) < 1e-6 * d["value"]
        assert "pinned host memory" in d["config"]["workload"]        # the headline loop: frames copied to the host
        for key in ("roofline", "rooflines_other", "value_in_hbm", "value_exact", "with_d2h", "cpu_baseline"):
            assert key not in d, key                                  # --full only
    out = [{n: np.load(d / (n + ".npy")) for n in ("render", "radii", "frames_rgb8")} for d in dumps]
    assert sorted(os.listdir(dumps[0])) == ["frames_rgb8.npy", "radii.npy", "render.npy"]
    render, radii, frames = out[0]["render"], out[0]["radii"], out[0]["frames_rgb8"]
    assert render.shape == (8, 9, 256, 256) and radii.shape == (8, 16384) and frames.shape == (8, 256, 256, 3)
    assert all(a.dtype == np.float32 for a in out[0].values())
    assert np.abs(render[:, :3]).max() > 0 and (radii > 0).any()       # something was rendered
    # the frames the host received are the 8-bit packing of the same step's planes
    assert np.array_equal(frames, (255 * np.clip(render[:, :3].transpose(0, 2, 3, 1), 0, 1)).astype(np.uint8).astype(np.float32))
    for n in out[0]:
        assert np.array_equal(out[0][n], out[1][n]), n                 # same arguments, same outputs
