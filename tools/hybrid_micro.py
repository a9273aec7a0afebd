"""What a sparse-dense hybrid search costs over the deep search it is built on, on one GPU.

  hybrid  1M x 512 float16 dotproduct rows, a sparse store of width 64 with 32 entries per row
          (indices stratified over a vocabulary of 32,000, so a row's entries ascend), queries of
          32 sparse entries, top-10, for 1 and for 64 queries per call: ``search_hybrid`` against
          ``search_deep`` with the same dense queries and the same k, timed in interleaved rounds:
          deep, hybrid, deep, ...  Quantity: wall ms per call (a synchronised window of --reps
          calls); median over the rounds with min-max, and the hybrid / deep ratio of the medians.

The yardstick is ``search_deep`` of the same build and the same process: the hybrid search is that
pipeline with the sparse add kernel between its score pass and its selection, and the deep calls
run the same instruction stream with or without a store.  Every line printed is one JSON record;
--out appends them to a file as well.  The part runs in a child process under its own time limit.
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
ROWS = 1_000_000
DIM = 512
WIDTH = 64
ROW_NNZ = 32
QUERY_NNZ = 32
STRATUM = 1000  # entry j of a row or a query lies in [j * STRATUM, (j + 1) * STRATUM)
K = 10
LIMITS = {"hybrid": 420}  # seconds per part


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def timed(fn, reps):
    import torch

    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def part_hybrid(args):
    import numpy as np
    import torch

    M = importlib.import_module(f"{PKG}.index")
    L = importlib.import_module(f"{PKG}._lib")
    rng = np.random.default_rng(5)
    dev = M.DeviceIndex(DIM, dtype="float16", capacity=ROWS, metric="dotproduct")
    dev.fill_random(2, 0, ROWS)
    dev.sparse_enable(WIDTH)
    # the store's rows as CSR straight to the library (a million Python dicts would take minutes)
    strata = (np.arange(ROW_NNZ, dtype=np.int64) * STRATUM)[None, :]
    idx = (strata + rng.integers(0, STRATUM, (ROWS, ROW_NNZ))).astype(np.uint32).reshape(-1)
    val = rng.standard_normal(ROWS * ROW_NNZ).astype(np.float32)
    off = np.arange(ROWS + 1, dtype=np.int64) * ROW_NNZ
    rows = np.arange(ROWS, dtype=np.int64)
    t0 = time.perf_counter()
    L.check(dev.lib.rc_index_sparse_write(dev.handle, rows.ctypes.data, off.ctypes.data, idx.ctypes.data, val.ctypes.data, ROWS,
                                          L.stream_ptr(None)))
    emit({"part": "hybrid", "what": "store write", "rows": ROWS, "width": WIDTH, "entries_per_row": ROW_NNZ,
          "store_bytes": 8 * WIDTH * ROWS, "seconds": time.perf_counter() - t0}, args.out)
    del idx, val, off, rows
    gen = torch.Generator(device="cuda").manual_seed(3)
    for nq in (1, 64):
        q = torch.randn(nq, DIM, device="cuda", generator=gen)
        sparse = []
        for _ in range(nq):
            qi = np.arange(QUERY_NNZ, dtype=np.int64) * STRATUM + rng.integers(0, STRATUM, QUERY_NNZ)
            sparse.append({"indices": qi.tolist(), "values": rng.standard_normal(QUERY_NNZ).astype(np.float32).tolist()})
        fns = {"deep": lambda: dev.search_deep(q, K, ROWS), "hybrid": lambda: dev.search_hybrid(q, K, ROWS, sparse)}
        for fn in fns.values():  # warm the kernels and the workspaces the timed window uses
            for _ in range(3):
                fn()
        moved = (dev.search_hybrid(q, K, ROWS, sparse)[1] != dev.search_deep(q, K, ROWS)[1]).any().item()
        t = {name: [] for name in fns}
        for _ in range(args.rounds):  # interleaved: deep, hybrid, deep, ...
            for name, fn in fns.items():
                t[name].append(timed(fn, args.reps))
        base = med(t["deep"])
        for name in fns:
            sm = sorted(t[name])
            emit({"part": "hybrid", "what": name, "rows": ROWS, "dim": DIM, "dtype": "float16", "metric": "dotproduct", "k": K,
                  "queries": nq, "width": WIDTH, "entries_per_row": ROW_NNZ, "entries_per_query": QUERY_NNZ,
                  "wall_ms": med(sm), "wall_ms_minmax": [sm[0], sm[-1]], "over_deep": med(sm) / base,
                  "results_differ_from_deep": bool(moved), "reps": args.reps, "rounds": args.rounds}, args.out)
    dev.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=["hybrid"], default=None,
                    help="run the part in this process (default: in a child process with a time limit)")
    ap.add_argument("--out", default=None, help="append the JSON records to this file")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if args.part is not None:
        part_hybrid(args)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--part", "hybrid", "--reps", str(args.reps), "--rounds", str(args.rounds)]
    if args.out:
        cmd += ["--out", args.out]
    subprocess.run(cmd, check=True, timeout=LIMITS["hybrid"])  # a failed or overrunning part ends the run


if __name__ == "__main__":
    main()
