"""bench.py on the GPU: a plain run prints the headline line only, and --dump-outputs writes the
last timed step's outputs (a small batch and two steps keep it to one short process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_last_step_outputs(cuda, tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", "8", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 2 and d["unit"] == "images/s" and d["dtype"] == "bf16" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0
    # value is the rate of the timed steps: batch / seconds per step
    assert abs(d["value"] - 8 / (d["ms_per_step"] / 1e3)) <= 1e-6 * d["value"]
    for moved in ("roofline", "gemms", "ingest", "jpeg", "latency", "search", "cpu_baseline"):
        assert moved not in d, f"{moved} belongs to --full"
    assert sorted(os.listdir(out)) == ["nrm.npy", "raw.npy"]
    raw, nrm = np.load(out / "raw.npy"), np.load(out / "nrm.npy")
    assert raw.dtype == np.float32 and nrm.dtype == np.float32
    assert raw.shape == (8, 768) and nrm.shape == (8, 768)
    assert np.isfinite(raw).all()
    # nrm is raw L2-normalised in float32 (u = 2^-24): the squared norm takes ~12 roundings per
    # lane and wave reduction (12 u, halved by the square root), the root, the reciprocal (<= 2.5 ulp)
    # and the product a few more: under 11 u = 6.6e-7 relative, on elements of magnitude <= 1
    want = raw / np.linalg.norm(raw.astype(np.float64), axis=1, keepdims=True)
    assert np.abs(nrm - want).max() <= 1e-6
