"""A plain bench.py run end to end: the lean result line, and --dump-outputs writing the last timed step's frame --
the same frame in every run, whatever the clock ramp rendered before the warmup steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_frame(tmp_path):
    import bench
    from reflaxman_amd import scenes
    from reflaxman_amd.render import DEFAULT_JITTER_SEED
    from helpers import gpu_render
    W, H, steps, warmup = 160, 90, 2, 1
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", str(warmup), "--width", str(W), "--height", str(H), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup and line["full"] is False
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    # value is traces per second of a timed step; both figures are rounded (ms_per_step to 1e-4 of ~5e-2 ms)
    assert line["value"] == pytest.approx(W * H / line["ms_per_step"] / 1e3, rel=1e-2)
    # what --full adds is absent from a plain line
    for k in ("cpu_baseline", "cpu_allcore", "roofline", "parity", "end_to_end_incl_d2h", "first_view", "c4_1gpu"):
        assert k not in line
    files = {f: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(files) == ["argb8.npy", "pixel_index.npy", "rgb.npy"] == sorted(line["outputs"]["files"])
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert np.array_equal(files["pixel_index.npy"], np.arange(W * H))
    # the frames from the reference's seeds on: warmup + steps of them, the last one dumped
    rgb, argb, rr = gpu_render(scenes.get_scene("synth16"), W, H, 8, frames=warmup + steps, sphere_seed=bench.SEED,
                               jitter_seed=DEFAULT_JITTER_SEED)
    rr.close()
    assert np.array_equal(files["rgb.npy"].view(np.uint32), rgb.reshape(-1, 3).view(np.uint32))
    a8 = files["argb8.npy"].astype(np.uint32)
    assert np.array_equal(a8[:, 0] << 24 | a8[:, 1] << 16 | a8[:, 2] << 8 | a8[:, 3], argb.reshape(-1).view(np.uint32))
