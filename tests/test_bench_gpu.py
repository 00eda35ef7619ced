"""GPU: bench.py as the driver calls it - a plain run prints one JSON line without the --full extras, and --dump-outputs writes
the last timed step's records, the same table on every run with the same arguments (seeded images and weights)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from facet_amd._lib import FE_FACE_FLOATS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, STEPS = 4, 2
ARGS = ["--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--batch", str(B), "--size", "256", "--microbatch", "8"]


def _bench(extra, cwd):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra, cwd=cwd, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_and_dumped_records(tmp_path):
    d = _bench(["--dump-outputs", str(tmp_path / "a")], tmp_path)
    assert d["steps"] == STEPS and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["metric"]
    assert abs(d["value"] - B / (d["ms_per_step"] * 1e-3)) < 0.02 * d["value"]
    assert "sub" not in d and "cpu_baseline" not in d and d["roofline"]["per_launch"] is None
    rec = np.load(tmp_path / "a" / "records.npy")
    assert rec.dtype == np.float32 and rec.shape == (B, 789 + 1 + 2 * FE_FACE_FLOATS)
    assert np.isfinite(rec).all() and rec[:, 0].std() > 0
    _bench(["--dump-outputs", str(tmp_path / "b")], tmp_path)
    assert np.array_equal(rec, np.load(tmp_path / "b" / "records.npy"))
