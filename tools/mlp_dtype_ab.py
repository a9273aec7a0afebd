"""Alternate mlp_dtype bf16 / mxfp8 at batch 256, parts = 2, in one process (GPU): images/s (kernel
timers off) and per-launch fc1 / fc2 times (rc_model_timing ids 1 and 7, in a pass of their own).

    python tools/mlp_dtype_ab.py        # log: profiles/mxfp8/mlp_dtype_ab.log
"""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import import_pkg  # noqa: E402

vit = import_pkg("vit")
B, RUNS, STEPS = 256, 6, 5
m = vit.VitMsnEmbedder(vit.random_state_dict(0), device=0, max_batch=B)
m.set_parts(2)
x = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B, 224, 224, 3), dtype=np.uint8)).cuda()
raw = torch.empty((B, 768), device="cuda")
nrm = torch.empty((B, 768), device="cuda")
res = {"bf16": {"ips": [], "fc1_us": [], "fc2_us": []}, "mxfp8": {"ips": [], "fc1_us": [], "fc2_us": []}}
for dt in ("bf16", "mxfp8"):  # warm up both
    m.set_mlp_dtype(dt)
    for _ in range(3):
        m.embed(x, out=(raw, nrm))
torch.cuda.synchronize()
for run in range(RUNS):
    for dt in ("bf16", "mxfp8"):
        m.set_mlp_dtype(dt)
        m.timing(False)
        m.embed(x, out=(raw, nrm))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            m.embed(x, out=(raw, nrm))
        torch.cuda.synchronize()
        res[dt]["ips"].append(B * STEPS / (time.perf_counter() - t0))
        m.timing(["fc1", "fc2"])
        m.timing_reset()
        for _ in range(2):
            m.embed(x, out=(raw, nrm))
        torch.cuda.synchronize()
        for k in ("fc1", "fc2"):
            ms, n, _ = m.timing_read(k)
            res[dt][k + "_us"].append(1e3 * ms / max(n, 1))
        print(run, dt, {k: round(v[-1], 1) for k, v in res[dt].items()}, flush=True)
summary = {dt: {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in r.items()} for dt, r in res.items()}
print(json.dumps(summary))
m.close()
