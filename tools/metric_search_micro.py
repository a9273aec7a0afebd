"""What the dotproduct and euclidean metrics cost against the cosine search of the same build, on
one GPU.  Two parts, each a child process of its own under its own time limit (a part that fails
or runs out of time ends the run):

  scan    the exact scan: 1M x 512 f32 and f16, one query, top-10, the three metrics switched on
          ONE populated index (rc_index_set_metric) and timed in interleaved rounds: cosine,
          dotproduct, euclidean, cosine, ...  Quantity: the scan kernel's time from the library's
          event timing (rc_index_timing), per call; median over the rounds.
  query1  the one-launch single-query path: top-5 over 10k x 768 f32 (tools/lat_probe.py's case),
          ShardSet.query_host without values, host latency per call (p50 of each round, median
          over the rounds), the same interleaving.

The yardstick is the cosine search of the same build and the same process (its kernels are
instruction-identical to the parent commit's: profiles/metrics/asm_diff.txt).  Every line printed
is one JSON record; --out appends them to a file as well.
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
ROWS, DIM = 1_000_000, 512
METRICS = ("cosine", "dotproduct", "euclidean")
LIMITS = {"scan": 300, "query1": 180}  # seconds per part


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def timed(dev, fn, reps):
    import torch

    torch.cuda.synchronize()
    dev.timing_read()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t) / reps * 1e3
    ms, _, _ = dev.timing_read()
    return wall, ms / reps


def part_scan(args):
    import torch

    M = importlib.import_module(f"{PKG}.index")
    for dtype in ("float32", "float16"):
        d = M.DeviceIndex(DIM, dtype=dtype, capacity=ROWS)
        d.fill_random(2, 0, ROWS)
        q = torch.randn(1, DIM, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        d.timing(True)
        fn = lambda: d.search(q, 10, ROWS, mode="scan")  # noqa: E731
        for m in METRICS:  # warm every kernel the timed window uses
            d.set_metric(m)
            for _ in range(5):
                fn()
        t = {m: [] for m in METRICS}
        for _ in range(args.rounds):  # interleaved: cosine, dotproduct, euclidean, cosine, ...
            for m in METRICS:
                d.set_metric(m)
                t[m].append(timed(d, fn, args.reps))
        el = 4 if dtype == "float32" else 2
        base = med(x[1] for x in t["cosine"])
        for m in METRICS:
            sm = sorted(x[1] for x in t[m])
            emit({"part": "scan", "dtype": dtype, "rows": ROWS, "dim": DIM, "k": 10, "metric": m, "scan_ms": med(sm),
                  "scan_ms_minmax": [sm[0], sm[-1]], "over_cosine": med(sm) / base, "wall_ms": med(x[0] for x in t[m]),
                  "GBps": ROWS * DIM * el / (med(sm) * 1e-3) / 1e9, "reps": args.reps, "rounds": args.rounds}, args.out)
        d.close()


def part_query1(args):
    import numpy as np
    import torch

    M = importlib.import_module(f"{PKG}.index")
    n, dim, k = 10000, 768, 5
    rng = np.random.default_rng(7)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    s = M.ShardSet(dim, dtype="float32", capacity_per_shard=n, devices=[0])
    s.upsert_rows(torch.from_numpy(X), torch.arange(n))
    q = np.ascontiguousarray(X[1234][None])
    fn = lambda: s.query_host(q, k, n, False)  # noqa: E731

    def p50(reps):
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return float(np.median(t)) * 1e3

    for m in METRICS:
        s.set_metric(m)
        for _ in range(50):
            fn()
    t = {m: [] for m in METRICS}
    for _ in range(args.rounds):
        for m in METRICS:
            s.set_metric(m)
            t[m].append(p50(args.reps * 10))
    base = med(t["cosine"])
    for m in METRICS:
        v = sorted(t[m])
        emit({"part": "query1", "dtype": "float32", "rows": n, "dim": dim, "k": k, "metric": m, "p50_ms": med(v),
              "p50_ms_minmax": [v[0], v[-1]], "over_cosine": med(v) / base, "reps": args.reps * 10, "rounds": args.rounds},
             args.out)
    s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=["scan", "query1"], default=None,
                    help="run one part in this process (default: every part, each in a child process with a time limit)")
    ap.add_argument("--parts", default="scan,query1")
    ap.add_argument("--out", default=None, help="append the JSON records to this file")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if args.part is not None:
        {"scan": part_scan, "query1": part_query1}[args.part](args)
        return
    for part in args.parts.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--reps", str(args.reps), "--rounds", str(args.rounds)]
        if args.out:
            cmd += ["--out", args.out]
        subprocess.run(cmd, check=True, timeout=LIMITS[part])  # a failed or overrunning part ends the run


if __name__ == "__main__":
    main()
