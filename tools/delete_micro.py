"""``Index.delete`` timings on one GPU against what the index offered before it: export the rows,
drop the deleted ones on the host, import the rest into a fresh index.

1M x 512 f16; one shard, three shards on the GPU (cross-shard pairs move in one launch), and three
shards with ``force_remote`` (cross-shard pairs take the pack / peer copy / unpack path of a
multi-GPU node); a uniformly random 0.1 %, 1 %, 10 % and 50 % of the ids deleted.  Each
configuration is a child process under its own time limit (one that fails or overruns ends the
run).  Per fraction the two methods alternate (delete, rebuild, delete, ...) on freshly filled
indexes; both end with the same ids on the same number of rows.

In the first round of every fraction the stored bytes are checked too: export_rows after the
delete equals the rows before it in the order plan_compaction predicts ("bytes_checked").

Every line printed is one JSON record (medians over --rounds); --out appends them to a file.
  delete_wall_ms   host clock around Index.delete(ids=...), which returns after the device moves
  plan_ms          of that: compaction.plan_compaction
  move_call_ms     of that: ShardSet.move_rows (list staging, launches, copies, synchronise)
  move_sync_ms     the same moves as one ShardSet.move_rows call on ready int64 tensors, staging
                   warm: validation, list staging, every launch and copy, one synchronise per
                   round - the device time of the sharded call plus its C++ host part (its
                   streams are the library's own, so no event pair of the caller's brackets them)
  kernel_ms        one shard only: the same moves as one rc_index_move_rows launch between two
                   events on the caller's stream (device time of move_rows_kernel alone)
  moved_rows, moved_MB (stored bytes read + written), kernel_GBps
  rebuild_wall_ms  export_rows + host drop + fresh Index + import_rows + the id maps
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
ROWS, DIM, DTYPE = 1_000_000, 512, "float16"
FRACTIONS = (0.001, 0.01, 0.1, 0.5)
CONFIGS = {"1": (1, False), "3": (3, False), "3remote": (3, True)}
LIMIT = 400  # seconds per configuration


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def filled_index(M, shards, remote, ids):
    """An Index of ROWS synthetic rows under the given ids (rows on the device, maps on the host)."""
    import torch

    idx = M.Index("delete-micro", dimension=DIM, dtype=DTYPE, capacity=ROWS, shards=shards)
    if remote:
        idx.shard_set.force_remote()
    for s in range(shards):
        idx.shard_set.shard(s).fill_random(11 + s, 0, idx.shard_set.shard_rows(s, ROWS))
    torch.cuda.synchronize()
    idx._ids = list(ids)
    idx._rows = {v: r for r, v in enumerate(idx._ids)}
    return idx


def rebuild(M, idx, dead, shards, remote):
    """The parent's way to the same result: rows out, dropped on the host, into a fresh index."""
    import numpy as np

    n = len(idx)
    rows, norms = idx.shard_set.export_rows(n)
    keep = np.ones(n, bool)
    keep[[idx._rows[i] for i in dead]] = False
    fresh = M.Index("delete-micro", dimension=DIM, dtype=DTYPE, capacity=ROWS, shards=shards)
    if remote:
        fresh.shard_set.force_remote()
    fresh.shard_set.import_rows(rows[keep], norms[keep])
    fresh._ids = [v for v, k in zip(idx._ids, keep.tolist()) if k]
    fresh._rows = {v: r for r, v in enumerate(fresh._ids)}
    return fresh


def part(args):
    import numpy as np
    import torch

    M = importlib.import_module(f"{PKG}.index")
    C = importlib.import_module(f"{PKG}.compaction")
    shards, remote = CONFIGS[args.config]
    ids = [f"id-{i:07d}" for i in range(ROWS)]
    el = 2
    idx = filled_index(M, shards, remote, ids)  # the fill is a function of (seed, row): the same rows every time
    rows0, norms0 = idx.shard_set.export_rows(ROWS)
    idx.close()
    for frac in FRACTIONS:
        rng = np.random.default_rng(int(frac * 1e6))
        dead = [ids[i] for i in rng.choice(ROWS, int(ROWS * frac), replace=False)]
        rec = {"delete_wall_ms": [], "plan_ms": [], "move_call_ms": [], "move_sync_ms": [], "kernel_ms": [],
               "rebuild_wall_ms": []}
        moved = 0
        for rnd in range(args.rounds):
            idx = filled_index(M, shards, remote, ids)
            src, dst = C.plan_compaction(ROWS, [idx._rows[i] for i in dead], shards)
            moved = len(src)
            if shards == 1 and moved:  # the kernel alone (the delete below repeats the same moves: same bytes)
                d = idx.shard_set.shard(0)
                s_t, d_t = torch.tensor(src, device=d.device), torch.tensor(dst, device=d.device)
                d.move_rows(s_t[:64], d_t[:64])  # first-launch cost stays out
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                d.move_rows(s_t, d_t)
                e1.record()
                torch.cuda.synchronize()
                rec["kernel_ms"].append(e0.elapsed_time(e1))
            if moved:  # the sharded call on ready tensors (the same moves again: the same bytes)
                s_h, d_h = torch.tensor(src), torch.tensor(dst)
                idx.shard_set.move_rows(s_h, d_h)  # staging and first launches stay out
                t = time.perf_counter()
                idx.shard_set.move_rows(s_h, d_h)
                rec["move_sync_ms"].append((time.perf_counter() - t) * 1e3)
            spent = {"plan": 0.0, "move": 0.0}
            plan0, move0 = C.plan_compaction, idx.shard_set.move_rows

            def plan(*a, **k):
                t = time.perf_counter()
                r = plan0(*a, **k)
                spent["plan"] += time.perf_counter() - t
                return r

            def move(*a, **k):
                t = time.perf_counter()
                move0(*a, **k)
                spent["move"] += time.perf_counter() - t

            C.plan_compaction, idx.shard_set.move_rows = plan, move
            try:
                t = time.perf_counter()
                idx.delete(ids=dead)
                rec["delete_wall_ms"].append((time.perf_counter() - t) * 1e3)
            finally:
                C.plan_compaction = plan0
                del idx.shard_set.move_rows
            rec["plan_ms"].append(spent["plan"] * 1e3)
            rec["move_call_ms"].append(spent["move"] * 1e3)
            kept = set(idx._ids)
            if rnd == 0:  # the stored bytes: the rows before the delete, in the order the plan predicts
                order = np.arange(ROWS)
                order[dst] = order[src]
                order = order[:ROWS - len(dead)]
                assert idx._ids == [ids[i] for i in order]
                got_r, got_n = idx.shard_set.export_rows(len(idx))
                assert np.array_equal(got_r, rows0[order]) and np.array_equal(got_n.view(np.uint32), norms0[order].view(np.uint32))
            idx.close()
            idx = filled_index(M, shards, remote, ids)
            t = time.perf_counter()
            fresh = rebuild(M, idx, dead, shards, remote)
            torch.cuda.synchronize()
            rec["rebuild_wall_ms"].append((time.perf_counter() - t) * 1e3)
            assert set(fresh._ids) == kept and len(fresh) == ROWS - len(dead)
            fresh.close()
            idx.close()
        mb = 2 * moved * DIM * el / 1e6
        out = {"shards": shards, "force_remote": remote, "rows": ROWS, "dim": DIM, "dtype": DTYPE, "fraction": frac,
               "deleted": len(dead), "moved_rows": moved, "moved_MB": mb, "rounds": args.rounds, "bytes_checked": True}
        for k, v in rec.items():
            out[k] = med(v) if v else None
            if v:
                out[k + "_minmax"] = [min(v), max(v)]
        out["kernel_GBps"] = mb / out["kernel_ms"] if out["kernel_ms"] else None
        out["delete_over_rebuild"] = out["delete_wall_ms"] / out["rebuild_wall_ms"]
        emit(out, args.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None,
                    help="run one configuration in this process (default: each in a child process with a time limit)")
    ap.add_argument("--configs", default="1,3,3remote")
    ap.add_argument("--out", default=None, help="append the JSON records to this file")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.config is not None:
        part(args)
        return
    for cfg in args.configs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--config", cfg, "--rounds", str(args.rounds)]
        if args.out:
            cmd += ["--out", args.out]
        subprocess.run(cmd, check=True, timeout=LIMIT)  # a failed or overrunning configuration ends the run


if __name__ == "__main__":
    main()
