"""bench.py as it is run for every change: a plain run times exactly --steps steps, prints the headline line, and
--dump-outputs writes what the last timed step computed (float32, seeded sample of the per-ray outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=300):
    cp = subprocess.run([sys.executable, "bench.py"] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert cp.returncode == 0, f"{args} exited with {cp.returncode}\n{cp.stdout[-2000:]}\n{cp.stderr[-4000:]}"
    lines = [ln for ln in cp.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, cp.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_step(tmp_path):
    out = _run(["--gpus", "1", "--steps", "4", "--warmup", "1", "--log2-pupil", "21", "--dump-outputs", str(tmp_path)])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 4 and out["repeats"] == 1 and len(out["repeats_ms_per_step"]) == 1
    assert out["full"] is False and out["also"] == {} and out["cpu_baseline"] is None and out["sweep"] is None
    assert out["value"] > 0 and out["ms_per_step"] > 0
    files = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(files) >= {"rms", "x", "y", "cx", "cy", "ok", "back", "grad_c", "grad_t", "grad_mu"}
    assert all(a.dtype == np.float32 for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    # 2^21 rays: the per-ray outputs are the seeded 2^20-ray sample
    assert all(files[k].shape == (1 << 20,) for k in ("x", "y", "cx", "cy", "ok", "back"))
    assert float(files["rms"][0]) == np.float32(out["config"]["rms"])
    assert np.isfinite(files["grad_c"]).all() and np.abs(files["grad_c"]).max() > 0
    assert set(np.unique(files["ok"])) <= {0.0, 1.0} and files["ok"].sum() > 0
