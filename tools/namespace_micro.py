"""Namespace (page-table scan) timings on one GPU.  Three parts, each a child process of its own
under its own time limit (a part that fails or runs out of time ends the run):

  scan    the paged scan against the contiguous scan of the same build, interleaved rounds:
          1,048,576 x 512 f32 and f16 (4096 pages), one query, top-10, the page list ascending
          (the same rows in the same order as the contiguous scan reads them) and shuffled;
  pool    a 4,096-vector and a 65,536-vector namespace (f16 x 512) on pages scattered through a
          pool of 1,048,576 rows, against (i) a dense index of the namespace's size (the floor),
          (ii) the same pool searched through the masked scan with the namespace's rows as the
          bitmap (the design the paged scan replaces) and (iii) the same namespace in a pool of
          4,194,304 rows (the time should follow the namespace, not the pool);
  query   Index.query p50 (top-5, 768 f32, 10,000 vectors, host in / host out) in a named
          namespace against the default one.

Every line printed is one JSON record; --out appends them to a file as well (default
profiles/namespaces/namespace_micro.jsonl).
Times: "scan_ms" is the library's own event timing of the scan kernel launches per call (median
of the rounds, with min / max), "wall_ms" a host clock around REPS calls ending in a device
synchronise, per call.
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
ROWS = 1 << 20
LIMITS = {"scan": 300, "pool": 300, "query": 200}  # seconds per part
DEFAULT_OUT = os.path.join(REPO, "profiles", "namespaces", "namespace_micro.jsonl")


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


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


def interleaved(dev, fns, reps, rounds):
    """{name: (median scan ms, [min, max], median wall ms)} of the calls fns, round-robin."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    got = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            got[name].append(timed(dev, fn, reps))
    out = {}
    for name, v in got.items():
        s, w = sorted(x[1] for x in v), sorted(x[0] for x in v)
        out[name] = (s[len(s) // 2], [s[0], s[-1]], w[len(w) // 2])
    return out


def record(part, res, extra, out):
    rec = dict(part=part, **extra)
    for name, (ms, mm, wall) in res.items():
        rec[name + "_scan_ms"] = ms
        rec[name + "_scan_ms_minmax"] = mm
        rec[name + "_wall_ms"] = wall
    emit(rec, out)
    return rec


def part_scan(args):
    import numpy as np
    import torch

    M = importlib.import_module(f"{PKG}.index")
    for dtype in ("float32", "float16"):
        d = M.DeviceIndex(DIM, dtype=dtype, capacity=ROWS)
        d.fill_random(2, 0, ROWS)
        q = torch.randn(1, DIM, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        d.timing(True)
        n_pages = ROWS // PAGE
        d.set_pages(0, np.arange(n_pages))
        d.set_pages(1, np.random.default_rng(5).permutation(n_pages))
        s0, r0 = d.search(q, 10, ROWS, mode="scan")
        s1, r1 = d.search_pages(q, 10, 0, ROWS)
        s2, _ = d.search_pages(q, 10, 1, ROWS)
        torch.cuda.synchronize()
        same = bool(torch.equal(s0, s1) and torch.equal(r0, r1) and torch.equal(s0, s2))
        res = interleaved(d, {"contiguous": lambda: d.search(q, 10, ROWS, mode="scan"),
                              "paged_ascending": lambda: d.search_pages(q, 10, 0, ROWS),
                              "paged_shuffled": lambda: d.search_pages(q, 10, 1, ROWS)}, args.reps, args.rounds)
        el = 4 if dtype == "float32" else 2
        record("scan", res, {"dtype": dtype, "rows": ROWS, "dim": DIM, "same_results": same,
                             "ascending_over_contiguous": res["paged_ascending"][0] / res["contiguous"][0],
                             "shuffled_over_contiguous": res["paged_shuffled"][0] / res["contiguous"][0],
                             "contiguous_GBps": ROWS * DIM * el / (res["contiguous"][0] * 1e-3) / 1e9,
                             "reps": args.reps, "rounds": args.rounds}, args.out)
        d.close()


def part_pool(args):
    import numpy as np
    import torch

    M = importlib.import_module(f"{PKG}.index")
    mf = importlib.import_module(f"{PKG}.metafilter")
    q = torch.randn(1, DIM, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    for pool_rows in (ROWS, 4 * ROWS):
        d = M.DeviceIndex(DIM, dtype="float16", capacity=pool_rows)
        d.fill_random(2, 0, pool_rows)
        d.timing(True)
        for n in (4096, 65536):
            # the namespace's pages: scattered through the whole pool, in no order
            page_list = np.random.default_rng(n).permutation(pool_rows // PAGE)[:n // PAGE]
            d.set_pages(0, page_list)
            fns = {"paged": lambda: d.search_pages(q, 10, 0, n),
                   "dense_floor": lambda: d.search(q, 10, n, mode="scan")}
            if pool_rows == ROWS:  # the rejected design: the whole pool under a namespace-shaped bitmap
                flags = np.zeros(pool_rows, bool)
                for p in page_list:
                    flags[p * PAGE:(p + 1) * PAGE] = True
                mask = torch.from_numpy(mf.pack_bits(flags).view(np.int32).copy()).to(d.device)
                fns["masked_pool"] = lambda: d.search(q, 10, pool_rows, mode="scan", mask=mask)
            res = interleaved(d, fns, args.reps, args.rounds)
            record("pool", res, {"dtype": "float16", "dim": DIM, "pool_rows": pool_rows, "namespace_rows": n,
                                 "paged_over_floor": res["paged"][0] / res["dense_floor"][0],
                                 "reps": args.reps, "rounds": args.rounds}, args.out)
        d.close()


def part_query(args):
    import numpy as np
    import torch

    M = importlib.import_module(f"{PKG}.index")
    n, dim = 10_000, 768
    X = torch.randn(n, dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    ix = M.Index("micro", dimension=dim, capacity=n)
    ids = [f"v{i}" for i in range(n)]
    ix.upsert_tensor(ids, X)
    ix.upsert_tensor(ids, X, namespace="tenant")
    qs = np.random.default_rng(2).standard_normal((64, dim)).astype(np.float32).tolist()
    for include_values in (False, True):
        p50 = {}
        for _ in range(args.rounds):
            for ns in ("", "tenant"):
                ts = []
                for i in range(args.calls):
                    t = time.perf_counter()
                    ix.query(vector=qs[i % 64], top_k=5, include_values=include_values, namespace=ns)
                    ts.append(time.perf_counter() - t)
                ts.sort()
                p50.setdefault(ns, []).append(ts[len(ts) // 2] * 1e3)
        med = {ns: sorted(v)[len(v) // 2] for ns, v in p50.items()}
        emit({"part": "query", "vectors": n, "dim": dim, "top_k": 5, "include_values": include_values,
              "default_p50_ms": med[""], "namespace_p50_ms": med["tenant"], "default_p50_ms_rounds": p50[""],
              "namespace_p50_ms_rounds": p50["tenant"], "calls": args.calls, "rounds": args.rounds}, args.out)
    ix.close()


PARTS = {"scan": part_scan, "pool": part_pool, "query": part_query}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=list(PARTS) + ["all"], default="all")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        PARTS[args.part](args)
        return
    for part in (PARTS if args.part == "all" else [args.part]):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--part", part, "--reps", str(args.reps), "--rounds",
               str(args.rounds), "--calls", str(args.calls), "--out", args.out]
        subprocess.run(cmd, check=True, timeout=LIMITS[part])


if __name__ == "__main__":
    main()
