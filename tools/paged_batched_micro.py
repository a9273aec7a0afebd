"""Row (d) of the namespace timings (tools/namespace_micro.py has (a)-(c)): the batched MFMA search
over pages on one GPU, against the two things it has to be judged by.

f16 x 512, top-10 and top-100, 16 / 64 / 1024 queries, a namespace of 65,536 / 262,144 / 1,048,576
positions on a shuffled page list scattered through a pool of 4,194,304 rows.  Per cell, interleaved
rounds of
  paged_mfma   DeviceIndex.search_pages(mode="mfma"): the page-table filter, rescore and fallback kernels;
  paged_scan   DeviceIndex.search_pages(mode="scan") of the same binary: what RC_SEARCH_AUTO chooses against;
  dense_mfma   DeviceIndex.search(mode="mfma") on a dense index of the namespace's size: the floor,
               the contiguous kernels.
"wall_ms" is a host clock around REPS calls ending in a device synchronise, per call: the median of
the rounds, with [min, max].  The three must return the same bits ("same_results").  Every line
printed is one JSON record; --out appends them to a file as well (default
profiles/paged_batched/paged_batched_micro.jsonl).  One child process per namespace size, each under
its own time limit.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "end-to-end-image-retrieval-service-with-k8s-jenkins_amd"
DIM, PAGE = 512, 256
POOL_ROWS = 1 << 22
SIZES = (65536, 262144, 1048576)
QUERIES = (16, 64, 1024)
TOPK = (10, 100)
LIMIT = 240  # seconds per namespace size
DEFAULT_OUT = os.path.join(REPO, "profiles", "paged_batched", "paged_batched_micro.jsonl")


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def wall(fn, reps):
    import torch

    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def interleaved(fns, reps, rounds):
    """{name: (median wall ms, [min, max])} of the calls fns, round-robin."""
    for fn in fns.values():
        fn()
        fn()
    got = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            got[name].append(wall(fn, reps[name]))
    return {name: (sorted(v)[len(v) // 2], [min(v), max(v)]) for name, v in got.items()}


def run_size(n, args):
    import numpy as np
    import torch

    M = importlib.import_module(f"{PKG}.index")
    pool = M.DeviceIndex(DIM, dtype="float16", capacity=POOL_ROWS)
    pool.fill_random(2, 0, POOL_ROWS)
    page_list = np.random.default_rng(n).permutation(POOL_ROWS // PAGE)[:n // PAGE]
    pool.set_pages(0, page_list)
    # the dense floor holds the same rows in position order, so the three paths must agree bit for bit
    dense = M.DeviceIndex(DIM, dtype="float16", capacity=n)
    for p0 in range(0, n // PAGE, 256):
        run = page_list[p0:p0 + 256]
        rows, norms = [], []
        for pg in run:
            r, nr = pool.export_rows(int(pg) * PAGE, PAGE)
            rows.append(r)
            norms.append(nr)
        dense.import_rows(p0 * PAGE, torch.cat(rows), torch.cat(norms))
    gen = torch.Generator(device="cuda").manual_seed(3)
    for nq in QUERIES:
        q = torch.randn(nq, DIM, device="cuda", generator=gen)
        for k in TOPK:
            fns = {"paged_mfma": lambda: pool.search_pages(q, k, 0, n, mode="mfma"),
                   "paged_scan": lambda: pool.search_pages(q, k, 0, n, mode="scan"),
                   "dense_mfma": lambda: dense.search(q, k, n, mode="mfma")}
            out = {name: fn() for name, fn in fns.items()}
            torch.cuda.synchronize()
            same = all(torch.equal(out["paged_mfma"][i], out[o][i]) for o in ("paged_scan", "dense_mfma") for i in (0, 1))
            reps = {"paged_mfma": args.reps, "dense_mfma": args.reps, "paged_scan": args.reps if nq <= 64 else max(1, args.reps // 10)}
            res = interleaved(fns, reps, args.rounds)
            rec = {"part": "paged_batched", "dtype": "float16", "dim": DIM, "pool_rows": POOL_ROWS, "positions": n,
                   "queries": nq, "top_k": k, "same_results": bool(same), "rounds": args.rounds, "reps": reps}
            for name, (ms, mm) in res.items():
                rec[name + "_wall_ms"] = ms
                rec[name + "_wall_ms_minmax"] = mm
            rec["mfma_below_scan"] = res["paged_mfma"][1][1] < res["paged_scan"][1][0]  # [min, max] wholly below
            rec["paged_over_dense"] = res["paged_mfma"][0] / res["dense_mfma"][0]
            emit(rec, args.out)
    dense.close()
    pool.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--size", type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.size:
        run_size(args.size, args)
        return
    for n in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--size", str(n), "--reps", str(args.reps), "--rounds", str(args.rounds),
               "--out", args.out]
        subprocess.run(cmd, check=True, timeout=LIMIT)


if __name__ == "__main__":
    main()
