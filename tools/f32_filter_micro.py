"""What the float32 filter (``filter="f32"``) buys a float32 index, on one GPU.

  throughput  1M x 512 and 1M x 768 float32 rows, top-100, 8 / 16 / 64 / 1024 queries per call,
              cosine and dotproduct: ``mode="mfma"`` under the "f32" filter against ``mode="scan"`` of
              the same index, and under cosine against ``mode="mfma"`` with the "i8" filter on the
              same rows.  Also the filter launches' own time (``gemm_timing_read``) as bytes of rows
              per second: the achieved share of HBM bandwidth when one query block reads them.
  crossover   16 384 ... 262 144 rows x 512 / 768, top-10, 8 and 16 queries: mfma against scan, the
              table ``RC_SEARCH_AUTO``'s corner for this filter is set from (kF32BatchMinPasses).

Quantity: wall ms per call (a synchronised window of --reps calls), timed in interleaved rounds
(scan, f32, i8, scan, ...); median over the rounds with min-max.  The yardstick is the scan of the
same build, index and process.  Every line printed is one JSON record; --out appends them to a file
as well.  Each part runs in a child process under its own time limit.
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
LIMITS = {"throughput": 500, "crossover": 300}  # seconds per part


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def timed(fn, reps):
    import torch

    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def rounds_of(fns, args, reps):
    """{name: sorted wall ms per call over the interleaved rounds}"""
    for fn in fns.values():  # warm the kernels and the workspaces the timed window uses
        fn()
    t = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            t[name].append(timed(fn, reps))
    return {name: sorted(v) for name, v in t.items()}


def part_throughput(args):
    import torch

    M = importlib.import_module(f"{PKG}.index")
    rows, k = 1_000_000, 100
    gen = torch.Generator(device="cuda").manual_seed(3)
    for dim in (512, 768):
        dev = M.DeviceIndex(dim, dtype="float32", capacity=rows)
        dev.fill_random(2, 0, rows)
        dev.set_filter("f32")
        dev8 = M.DeviceIndex(dim, dtype="float32", capacity=rows)
        dev8.fill_random(2, 0, rows)
        dev8.set_filter("i8")
        for metric in ("cosine", "dotproduct"):
            dev.set_metric(metric)
            for nq in (8, 16, 64, 1024):
                q = torch.randn(nq, dim, device="cuda", generator=gen)
                fns = {"scan": lambda: dev.search(q, k, rows, mode="scan"), "f32": lambda: dev.search(q, k, rows, mode="mfma")}
                if metric == "cosine":
                    fns["i8"] = lambda: dev8.search(q, k, rows, mode="mfma")
                t = rounds_of(fns, args, max(2, args.reps // (1 + nq // 64)))
                dev.timing(True)
                dev.gemm_timing_read()
                dev.search(q, k, rows, mode="mfma")
                torch.cuda.synchronize()
                ms, launches, _, fallbacks = dev.gemm_timing_read()
                dev.timing(False)
                for name, sm in t.items():
                    emit({"part": "throughput", "what": name, "rows": rows, "dim": dim, "metric": metric, "k": k, "queries": nq,
                          "wall_ms": sm[len(sm) // 2], "wall_ms_minmax": [sm[0], sm[-1]],
                          "scan_over_this": t["scan"][len(sm) // 2] / sm[len(sm) // 2], "rounds": args.rounds}, args.out)
                emit({"part": "throughput", "what": "f32 filter launches", "dim": dim, "metric": metric, "queries": nq,
                      "filter_ms": ms, "launches": launches, "fallbacks": fallbacks,
                      "row_bytes_per_s": (rows - 4096) * dim * 4 / (ms * 1e-3) if ms > 0 else None}, args.out)
            dev.set_metric("cosine")
        dev.close()
        dev8.close()


def part_crossover(args):
    import torch

    M = importlib.import_module(f"{PKG}.index")
    k = 10
    gen = torch.Generator(device="cuda").manual_seed(4)
    for dim in (512, 768):
        dev = M.DeviceIndex(dim, dtype="float32", capacity=262_144)
        dev.fill_random(2, 0, 262_144)
        dev.set_filter("f32")
        for metric in ("cosine", "dotproduct"):
            dev.set_metric(metric)
            for rows in (16_384, 32_768, 65_536, 131_072, 262_144):
                for nq in (8, 16):
                    q = torch.randn(nq, dim, device="cuda", generator=gen)
                    t = rounds_of({"scan": lambda: dev.search(q, k, rows, mode="scan"),
                                   "f32": lambda: dev.search(q, k, rows, mode="mfma")}, args, args.reps)
                    m = {name: sm[len(sm) // 2] for name, sm in t.items()}
                    emit({"part": "crossover", "rows": rows, "dim": dim, "metric": metric, "k": k, "queries": nq, "scan_ms": m["scan"],
                          "scan_ms_minmax": [t["scan"][0], t["scan"][-1]], "f32_ms": m["f32"], "f32_ms_minmax": [t["f32"][0], t["f32"][-1]],
                          "scan_over_f32": m["scan"] / m["f32"], "rounds": args.rounds}, args.out)
        dev.close()


PARTS = {"throughput": part_throughput, "crossover": part_crossover}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=sorted(PARTS), default=None,
                    help="run one part in this process (default: every part, each in a child process with a time limit)")
    ap.add_argument("--crossover", action="store_true", help="the crossover part only")
    ap.add_argument("--out", default=None, help="append the JSON records to this file")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.part is not None:
        PARTS[args.part](args)
        return
    for part in (["crossover"] if args.crossover else ["throughput", "crossover"]):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--reps", str(args.reps), "--rounds", str(args.rounds)]
        if args.out:
            cmd += ["--out", args.out]
        subprocess.run(cmd, check=True, timeout=LIMITS[part])  # a failed or overrunning part ends the run


if __name__ == "__main__":
    main()
