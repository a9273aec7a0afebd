"""What a metadata-filter bitmap costs on a cache miss: the host path (``metafilter.build_bitmap``, a
Python pass over every row's metadata — the index's only path before ``metadata_config``) against
the device path (``metacolumns``: the filter compiled to a program, ``rc_meta_eval`` over the typed
columns, the bitmap and count copied back).

What is timed is ``Index._bitmap_locked(filter)`` on a miss, forced by bumping the generation, with
a host clock; the device path ends in the synchronising copy of the bitmap, so the clock covers the
kernel.  Both paths run in the same process on the same index (``metacolumns.DEVICE_MIN_ROWS`` picks
the path), in interleaved rounds (host, device, host, ...), after one untimed miss each.  In the
first round the two bitmaps and counts are compared ("checked").  The host path is the yardstick: it
is the code an index without ``metadata_config`` runs.

1,000 / 10,000 / 100,000 / 1,000,000 rows x 64 f16 (the vectors play no part), three indexed fields
(a string of 8 values, an integer below 100, a boolean; each absent in 30 % of the rows), and three
filters: one leaf, four leaves over two fields, an ``$in`` of 16.  Each row count is a child process
under its own time limit (one that fails or overruns ends the run).

Every line printed is one JSON record (median over --rounds, with [min, max]); --out appends them
to a file.
"""
import argparse
import importlib
import json
import os
import random
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "end-to-end-image-retrieval-service-with-k8s-jenkins_amd"
ROWS = (1_000, 10_000, 100_000, 1_000_000)
DIM, DTYPE = 64, "float16"
FIELDS = ["color", "size", "flag"]
COLORS = ["red", "green", "blue", "cyan", "magenta", "yellow", "black", "white"]
FILTERS = {
    "one_leaf": {"size": {"$lt": 25}},
    "four_leaves_two_fields": {"size": {"$gte": 10, "$lt": 60}, "color": {"$ne": "red", "$exists": True}},
    "in_16": {"size": {"$in": list(range(3, 51, 3))}},
}
LIMIT = 600  # seconds per row count


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def metadata(n, seed=7):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        md = {}
        if rng.random() >= 0.3:
            md["color"] = rng.choice(COLORS)
        if rng.random() >= 0.3:
            md["size"] = rng.randrange(100)
        if rng.random() >= 0.3:
            md["flag"] = rng.random() < 0.5
        out.append(md)
    return out


def part(args):
    import numpy as np
    import torch

    M = importlib.import_module(f"{PKG}.index")
    MC = importlib.import_module(f"{PKG}.metacolumns")
    n = args.rows
    idx = M.Index("metafilter-micro", dimension=DIM, dtype=DTYPE, capacity=n, metadata_config={"indexed": FIELDS})
    metas = metadata(n)
    t0 = time.perf_counter()
    for i in range(0, n, 50_000):
        m = min(50_000, n - i)
        idx.upsert_tensor([f"id-{j:07d}" for j in range(i, i + m)], torch.randn((m, DIM), device="cuda"), metas[i:i + m])
    fill_s = time.perf_counter() - t0

    def miss(flt, device):
        """One cache miss on the chosen path: (milliseconds, (bitmap, count))."""
        MC.DEVICE_MIN_ROWS = 0 if device else 1 << 62
        with idx._mu:
            idx._gen += 1
            t = time.perf_counter()
            hit = idx._bitmap_locked(flt)
            return (time.perf_counter() - t) * 1e3, hit

    for name, flt in FILTERS.items():
        program = idx._fields.program(flt)
        assert program is not None
        before = idx.metadata_index_stats()
        miss(flt, False), miss(flt, True)  # untimed: first launch, allocator, code paths
        host, dev, checked = [], [], False
        for rnd in range(args.rounds):
            th, bh = miss(flt, False)
            td, bd = miss(flt, True)
            host.append(th)
            dev.append(td)
            if rnd == 0:
                assert bh[0].dtype == bd[0].dtype and np.array_equal(bh[0], bd[0]) and bh[1] == bd[1]
                checked = True
        after = idx.metadata_index_stats()
        assert after["host_evals"] - before["host_evals"] == args.rounds + 1 == after["device_evals"] - before["device_evals"]
        leaves = int((program[:, 0] & 0xFF <= MC.OP_NOT_EXISTS).sum())
        fields = len({int(w >> 8) & 0xFF for w in program[:, 0].tolist() if (w & 0xFF) <= MC.OP_NOT_EXISTS})
        emit({"rows": n, "filter": name, "leaves": leaves, "fields": fields, "instructions": int(program.shape[0]),
              "eligible": int(bd[1]), "rounds": args.rounds, "checked": checked,
              "host_ms": med(host), "host_ms_minmax": [min(host), max(host)],
              "device_ms": med(dev), "device_ms_minmax": [min(dev), max(dev)],
              "host_over_device": med(host) / med(dev), "device_wholly_below_host": max(dev) < min(host),
              "column_bytes_read": 9 * fields * n, "fill_s": fill_s}, args.out)
    idx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=None, help="run one row count in this process (default: each in a child "
                    "process with a time limit)")
    ap.add_argument("--sizes", default=",".join(map(str, ROWS)))
    ap.add_argument("--out", default=None, help="append the JSON records to this file")
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    if args.rows is not None:
        part(args)
        return
    for n in args.sizes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--rows", n, "--rounds", str(args.rounds)]
        if args.out:
            cmd += ["--out", args.out]
        subprocess.run(cmd, check=True, timeout=LIMIT)  # a failed or overrunning row count ends the run


if __name__ == "__main__":
    main()
