"""What the metric filter (rc_index_set_filter(RC_FILTER_METRIC)) buys and costs, on one GPU and
one build.  Two parts, each a child process of its own under its own time limit (a part that fails
or runs out of time ends the run):

  batch   1M x 512 and 1M x 768 f16 rows with lognormal norms (fill_random's directions, norms
          multiplied by exp(normal(0, 1))), batches of 256 queries x top-100 and 16 x top-10.  On
          ONE populated index, interleaved rounds of: the metric scan (what a batch cost before:
          one pass per query; its kernels are instruction-identical to the parent commit's), the
          batched search under the metric, and the batched search under cosine (the native cosine
          filter launch on the same rows: the yardstick of the metric epilogue).  Quantities per
          batch: wall ms (synchronised), the filter launches' device ms (rc_index_gemm_timing_read)
          and the fallback count; median over the rounds with min-max.
  corner  where "auto" switches: 8 and 16 queries x top-10 over 65 536, 131 072 and 262 144 rows x
          256 / 512 / 768, batched search against scan, wall ms per call.

Every line printed is one JSON record; --out appends them to a file as well.
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
LIMITS = {"batch": 420, "corner": 240}  # seconds per part


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def stat(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def populate(M, dim, rows, seed=2):
    """fill_random's directions with lognormal norms: the three metrics' top-k differ."""
    import torch

    d = M.DeviceIndex(dim, dtype="float16", capacity=rows)
    d.fill_random(seed, 0, rows)
    g = torch.Generator(device="cuda").manual_seed(5)
    step = 1 << 18
    for r0 in range(0, rows, step):
        n = min(step, rows - r0)
        bits, norms = d.export_rows(r0, n)
        d.import_rows(r0, bits, norms * torch.exp(torch.randn(n, device="cuda", generator=g)))
    d.set_filter("metric")
    return d


def timed(dev, fn, reps):
    """(wall ms, filter device ms, fallbacks) per call"""
    import torch

    torch.cuda.synchronize()
    dev.gemm_timing_read()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t) / reps * 1e3
    ms, _, _, fb = dev.gemm_timing_read()
    return wall, ms / reps, fb / reps


def part_batch(args):
    import torch

    M = importlib.import_module(f"{PKG}.index")
    for dim in (512, 768):
        d = populate(M, dim, ROWS)
        d.timing(True)
        for nq, k in ((256, 100), (16, 10)):
            q = torch.randn(nq, dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 3.0
            for metric in ("dotproduct", "euclidean"):
                arms = {"scan": (metric, "scan", max(1, args.reps // 8)), "mfma": (metric, "mfma", args.reps),
                        "cosine_mfma": ("cosine", "mfma", args.reps)}
                for m, mode, _ in arms.values():  # warm every kernel the timed window uses
                    d.set_metric(m)
                    d.search(q, k, ROWS, mode=mode)
                t = {a: [] for a in arms}
                for _ in range(args.rounds):  # interleaved: scan, mfma, cosine mfma, scan, ...
                    for a, (m, mode, reps) in arms.items():
                        d.set_metric(m)
                        t[a].append(timed(d, lambda: d.search(q, k, ROWS, mode=mode), reps))
                wall = {a: stat([x[0] for x in t[a]]) for a in arms}
                filt = {a: stat([x[1] for x in t[a]]) for a in arms}
                emit({"part": "batch", "dtype": "float16", "rows": ROWS, "dim": dim, "nq": nq, "k": k, "metric": metric,
                      "wall_ms": wall, "filter_ms": {a: filt[a] for a in ("mfma", "cosine_mfma")},
                      "fallbacks_per_call": {a: max(x[2] for x in t[a]) for a in ("mfma", "cosine_mfma")},
                      "scan_over_mfma_wall": wall["scan"]["median"] / wall["mfma"]["median"],
                      "metric_over_cosine_filter": filt["mfma"]["median"] / filt["cosine_mfma"]["median"],
                      "metric_over_cosine_wall": wall["mfma"]["median"] / wall["cosine_mfma"]["median"],
                      "reps": args.reps, "rounds": args.rounds}, args.out)
        d.timing(False)
        d.set_metric("cosine")
        d.close()


def part_corner(args):
    import torch

    M = importlib.import_module(f"{PKG}.index")
    k = 10
    for dim in (256, 512, 768):
        d = populate(M, dim, 262_144)
        for rows in (65_536, 131_072, 262_144):
            for nq in (8, 16):
                q = torch.randn(nq, dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 3.0
                for metric in ("dotproduct", "euclidean"):
                    d.set_metric(metric)
                    for mode in ("scan", "mfma"):
                        d.search(q, k, rows, mode=mode)
                    t = {"scan": [], "mfma": []}
                    for _ in range(args.rounds):
                        for mode in t:
                            t[mode].append(timed(d, lambda: d.search(q, k, rows, mode=mode), args.reps)[0])
                    w = {mode: stat(t[mode]) for mode in t}
                    emit({"part": "corner", "dtype": "float16", "rows": rows, "dim": dim, "nq": nq, "k": k, "metric": metric,
                          "wall_ms": w, "scan_over_mfma_wall": w["scan"]["median"] / w["mfma"]["median"], "reps": args.reps,
                          "rounds": args.rounds}, args.out)
        d.set_metric("cosine")
        d.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=["batch", "corner"], default=None,
                    help="run one part in this process (default: every part, each in a child process with a time limit)")
    ap.add_argument("--parts", default="batch,corner")
    ap.add_argument("--out", default=None, help="append the JSON records to this file")
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.part is not None:
        {"batch": part_batch, "corner": part_corner}[args.part](args)
        return
    for part in args.parts.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--reps", str(args.reps), "--rounds", str(args.rounds)]
        if args.out:
            cmd += ["--out", args.out]
        subprocess.run(cmd, check=True, timeout=LIMITS[part])  # a failed or overrunning part ends the run


if __name__ == "__main__":
    main()
