"""Masked (metadata-filtered) search timings on one GPU.  Four parts, each a child process of its
own under its own time limit (a part that fails or runs out of time ends the run):

  scan    the masked scan against the unmasked scan of the same build, interleaved: 1M x 512 f32
          and f16, one query, top-10, eligible shares 1.0 / 0.5 / 0.1 / 0.01 / 0.001, uniformly
          random and clustered (one contiguous run of eligible rows);
  parent  the unmasked scan of this build against another build of the library (--parent-lib,
          e.g. the parent commit's), alternating fresh processes;
  mfma    the masked MFMA path against the masked multi-query scan: 1M x 512 f16, 256 queries x
          top-100, shares 1.0 / 0.5 / 0.1 (and 0.35, 0.25, 0.01) — the crossover behind
          index.MASKED_MFMA_MIN_SHARE;
  maskfilter  the mask inside the filter GEMM (mode "mfma_masked") against the masked scan and
          against "mfma" (mask at rescoring only), interleaved, results compared bit for bit in every
          row.  "table": 1M x 512 f16, 256 queries x top-100, shares 1.0 ... 0.001 random and 0.1 /
          0.01 clustered, with the queries that fell back.  "grid": "mfma_masked" against the masked
          scan at 16 / 32 / 64 / 256 queries x top-10 / top-100, shares 0.25 ... 0.001, over the
          first 65,536, 1M and 16M rows of one index (--grid-rows; 32 and 256 queries only past
          1M rows) — what index.Index._masked_mode's rule below MASKED_MFMA_MIN_SHARE is read from.

Every line printed is one JSON record; --out appends them to a file as well.
Times: "wall_ms" is a host clock around REPS calls ending in a device synchronise, per call;
"scan_ms" is the library's own event timing of the scan kernel launches, per call.
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
SHARES = (1.0, 0.5, 0.1, 0.01, 0.001)
LIMITS = {"scan": 420, "parent": 480, "mfma": 300, "maskfilter": 420}  # seconds per part


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def make_mask(n, share, kind, seed, device):
    import numpy as np
    import torch

    mf = importlib.import_module(f"{PKG}.metafilter")
    if share >= 1.0:
        flags = np.ones(n, bool)
    elif kind == "random":
        flags = np.random.default_rng(seed).random(n) < share
    else:  # clustered: one contiguous run, not aligned to anything
        m = max(1, int(round(n * share)))
        start = (n - m) // 3 + 5
        flags = np.zeros(n, bool)
        flags[start:start + m] = True
    words = mf.pack_bits(flags)
    return torch.from_numpy(words.view(np.int32).copy()).to(device), int(flags.sum())


def timed(dev, fn, reps):
    import torch

    torch.cuda.synchronize()
    dev.timing_read()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t) / reps * 1e3
    ms, cnt, _ = dev.timing_read()
    return wall, ms / reps


def part_scan(args):
    import torch

    M = importlib.import_module(f"{PKG}.index")
    reps, rounds = args.reps, args.rounds
    for dtype in ("float32", "float16"):
        d = M.DeviceIndex(DIM, dtype=dtype, capacity=ROWS)
        d.fill_random(2, 0, ROWS)
        q = torch.randn(1, DIM, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        d.timing(True)
        el = 4 if dtype == "float32" else 2
        for share in SHARES:
            for kind in (("random",) if share >= 1.0 else ("random", "clustered")):
                mask, eligible = make_mask(ROWS, share, kind, 7, d.device)
                base = lambda: d.search(q, 10, ROWS, mode="scan")  # noqa: E731
                masked = lambda: d.search(q, 10, ROWS, mode="scan", mask=mask)  # noqa: E731
                for _ in range(3):
                    base()
                    masked()
                u, m = [], []
                for _ in range(rounds):  # interleaved: unmasked, masked, unmasked, ...
                    u.append(timed(d, base, reps))
                    m.append(timed(d, masked, reps))
                us, ms_ = sorted(x[1] for x in u), sorted(x[1] for x in m)
                uw, mw = sorted(x[0] for x in u), sorted(x[0] for x in m)
                med = lambda v: v[len(v) // 2]  # noqa: E731
                emit({"part": "scan", "dtype": dtype, "rows": ROWS, "dim": DIM, "share": share, "kind": kind,
                      "eligible": eligible, "unmasked_scan_ms": med(us), "masked_scan_ms": med(ms_),
                      "masked_over_unmasked": med(ms_) / med(us), "unmasked_scan_ms_minmax": [us[0], us[-1]],
                      "masked_scan_ms_minmax": [ms_[0], ms_[-1]], "unmasked_wall_ms": med(uw), "masked_wall_ms": med(mw),
                      "unmasked_GBps": ROWS * DIM * el / (med(us) * 1e-3) / 1e9, "reps": reps, "rounds": rounds}, args.out)
        d.close()


def part_parent_child(args):
    import torch

    M = importlib.import_module(f"{PKG}.index")
    for dtype in ("float32", "float16"):
        d = M.DeviceIndex(DIM, dtype=dtype, capacity=ROWS)
        d.fill_random(2, 0, ROWS)
        q = torch.randn(1, DIM, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        d.timing(True)
        fn = lambda: d.search(q, 10, ROWS, mode="scan")  # noqa: E731
        for _ in range(5):
            fn()
        r = sorted(timed(d, fn, args.reps)[1] for _ in range(args.rounds))
        emit({"part": "parent", "build": args.label, "dtype": dtype, "rows": ROWS, "unmasked_scan_ms": r[len(r) // 2],
              "minmax": [r[0], r[-1]]}, args.out)
        d.close()


def part_parent(args):
    if not args.parent_lib:
        emit({"part": "parent", "skipped": "no --parent-lib given"}, args.out)
        return
    for i in range(args.alternations):
        for label, lib in (("parent", args.parent_lib), ("this", None)):
            env = dict(os.environ)
            env.pop("RC_LIB_PATH", None)
            if lib:
                env["RC_LIB_PATH"] = os.path.abspath(lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--part", "parent-child", "--label", label, "--reps",
                   str(args.reps), "--rounds", str(args.rounds)] + (["--out", args.out] if args.out else [])
            subprocess.run(cmd, env=env, check=True, timeout=LIMITS["parent"] // (2 * args.alternations))


def part_mfma(args):
    import torch

    M = importlib.import_module(f"{PKG}.index")
    nq, k = 256, 100
    d = M.DeviceIndex(DIM, dtype="float16", capacity=ROWS)
    d.fill_random(4, 0, ROWS)
    Q = torch.randn(nq, DIM, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    d.timing(True)
    for share in (1.0, 0.5, 0.35, 0.25, 0.1, 0.01):
        mask, eligible = make_mask(ROWS, share, "random", 9, d.device)
        scan = lambda: d.search(Q, k, ROWS, mode="scan", mask=mask)  # noqa: E731
        mfma = lambda: d.search(Q, k, ROWS, mode="mfma", mask=mask)  # noqa: E731
        s0, r0 = scan()
        s1, r1 = mfma()
        torch.cuda.synchronize()
        same = bool(torch.equal(s0, s1) and torch.equal(r0, r1))
        d.gemm_timing_read()
        sw, mw = [], []
        for _ in range(args.rounds):
            sw.append(timed(d, scan, 2)[0])
            mw.append(timed(d, mfma, 4)[0])
        fallbacks = d.gemm_timing_read()[3]
        sw.sort()
        mw.sort()
        emit({"part": "mfma", "dtype": "float16", "rows": ROWS, "nq": nq, "k": k, "share": share, "eligible": eligible,
              "masked_scan_ms_per_batch": sw[len(sw) // 2], "masked_mfma_ms_per_batch": mw[len(mw) // 2],
              "mfma_over_scan": mw[len(mw) // 2] / sw[len(sw) // 2], "scan_minmax": [sw[0], sw[-1]],
              "mfma_minmax": [mw[0], mw[-1]], "fallback_queries_per_batch": fallbacks / (4 * args.rounds),
              "results_equal": same}, args.out)
    d.close()


def part_maskfilter(args):
    import torch

    M = importlib.import_module(f"{PKG}.index")
    grid_rows = [int(r) for r in args.grid_rows.split(",")]
    cap = max([ROWS] + grid_rows)
    d = M.DeviceIndex(DIM, dtype="float16", capacity=cap)
    d.fill_random(4, 0, cap)
    Qall = torch.randn(256, DIM, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    d.timing(True)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731

    def cell(what, rows, nq, k, share, kind, modes):
        mask, eligible = make_mask(rows, share, kind, 9, d.device)
        Q = Qall[:nq]
        fns = {m: (lambda m=m: d.search(Q, k, rows, mode=m, mask=mask)) for m in modes}
        ref = fns["scan"]()
        torch.cuda.synchronize()
        rec = {"part": "maskfilter", "what": what, "dtype": "float16", "rows": rows, "dim": DIM, "nq": nq, "k": k,
               "share": share, "kind": kind, "eligible": eligible}
        for m in modes[1:]:  # bit equality with the masked scan, and the queries that fell back in one call
            d.gemm_timing_read()
            got = fns[m]()
            torch.cuda.synchronize()
            rec[m + "_equals_scan"] = bool(torch.equal(ref[0].view(torch.int32), got[0].view(torch.int32)) and
                                           torch.equal(ref[1], got[1]))
            rec[m + "_fallback_queries"] = d.gemm_timing_read()[3]
        wall = {m: [] for m in modes}
        for _ in range(args.rounds):  # interleaved: scan, mfma, mfma_masked, scan, ...
            for m in modes:
                wall[m].append(timed(d, fns[m], 2 if m == "scan" else 4)[0])
        for m in modes:
            rec[m + "_ms_per_batch"] = med(wall[m])
            rec[m + "_minmax"] = [min(wall[m]), max(wall[m])]
        rec["scan_over_mfma_masked"] = rec["scan_ms_per_batch"] / rec["mfma_masked_ms_per_batch"]
        emit(rec, args.out)

    for share, kind in [(1.0, "random"), (0.5, "random"), (0.35, "random"), (0.25, "random"), (0.1, "random"),
                        (0.01, "random"), (0.001, "random"), (0.1, "clustered"), (0.01, "clustered")]:
        cell("table", ROWS, 256, 100, share, kind, ["scan", "mfma", "mfma_masked"])
    for rows in grid_rows:
        for nq in ((16, 32, 64, 256) if rows <= ROWS else (32, 256)):
            for k in (10, 100):
                for share in (0.25, 0.1, 0.01, 0.001):
                    cell("grid", rows, nq, k, share, "random", ["scan", "mfma_masked"])
    d.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=["scan", "parent", "parent-child", "mfma", "maskfilter"], default=None,
                    help="run one part in this process (default: every part, each in a child process with a time limit)")
    ap.add_argument("--parts", default="scan,parent,mfma,maskfilter")
    ap.add_argument("--parent-lib", default=None, help="another build of libretrieval_core.so to compare the unmasked scan with")
    ap.add_argument("--out", default=None, help="append the JSON records to this file")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--label", default="this")
    ap.add_argument("--grid-rows", default="65536,1000000,16000000", help="maskfilter: the grid's row counts")
    args = ap.parse_args()
    if args.part is not None:
        {"scan": part_scan, "parent": part_parent, "parent-child": part_parent_child, "mfma": part_mfma,
         "maskfilter": part_maskfilter}[args.part](args)
        return
    for part in args.parts.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--reps", str(args.reps), "--rounds", str(args.rounds),
               "--alternations", str(args.alternations)]
        if args.parent_lib:
            cmd += ["--parent-lib", args.parent_lib]
        if args.out:
            cmd += ["--out", args.out]
        if part == "maskfilter":
            cmd += ["--grid-rows", args.grid_rows]
        subprocess.run(cmd, check=True, timeout=LIMITS[part])  # a failed or overrunning part ends the run


if __name__ == "__main__":
    main()
