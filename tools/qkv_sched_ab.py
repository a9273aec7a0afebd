"""Schedule variants of the fused QKV + attention kernel (csrc/qkv_attention.h), in one process.

Diagnostic build (tools/build_diag.sh):
    RC_LIB_PATH=...lib/diag/libretrieval_core.so python tools/qkv_sched_ab.py [--out FILE.jsonl]

For the batch-256 embed at parts = 1 (12 seeded layers, 11 fused launches per step):
  bits    every variant's (raw, nrm) against fusion off, bitwise
  ab      ROUNDS rounds over the variants in turn: HIP-event time per fused launch and ms per step
  phases  per-workgroup phase times from the kernel's s_memrealtime stamps (100 MHz): prologue (block
          entry -> K loop start), K loop, epilogue (-> the barrier behind the Q/K/V stores), attention
          (-> the last wave's end), and each wave's attention time
Variant bits: 1 epilogue loads hoisted, 2 K-step DMA among the MFMAs behind counted LDS waits;
-1 is the library's product kernel.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.weights import seeded_vit_msn_weights  # noqa: E402

PKG = "end-to-end-image-retrieval-service-with-k8s-jenkins_amd"
TICK_US = 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="0,1,2,3,-1", help="empty: phases only")
    ap.add_argument("--phase-variants", default="0,1,2,3")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    variants = [int(v) for v in args.variants.split(",") if v]
    L = importlib.import_module(f"{PKG}._lib")
    vit = importlib.import_module(f"{PKG}.vit")
    raw_lib = C.CDLL(L.LIB_PATH)
    raw_lib.rc_diag_set_stamps.argtypes = [C.c_void_p]
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    dev = torch.device("cuda", 0)
    m = vit.VitMsnEmbedder(seeded_vit_msn_weights(1907), device=0, max_batch=args.batch)
    m.set_parts(1)
    rng = np.random.default_rng(5)
    imgs = torch.from_numpy(rng.integers(0, 256, (args.batch, 224, 224, 3), dtype=np.uint8)).to(dev)

    def run():
        r, v = m.embed(imgs)
        torch.cuda.synchronize()
        return r, v

    m.set_qkv_fusion(0)
    ref = tuple(t.clone() for t in run())
    m.set_qkv_fusion(2)
    for v in variants:
        m.set_qkv_sched(v)
        r, n = run()
        emit({"kind": "bits", "variant": v, "equal_unfused": bool(torch.equal(r, ref[0]) and torch.equal(n, ref[1]))})

    m.timing(["qkv"])
    for rnd in range(args.rounds):
        for v in variants:
            m.set_qkv_sched(v)
            run()
            m.timing_reset()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                m.embed(imgs)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.steps
            ms, n, _ = m.timing_read("qkv")
            emit({"kind": "ab", "round": rnd, "variant": v, "qkv_us": round(ms / max(n, 1) * 1e3, 2), "launches": n,
                  "step_ms": round(dt * 1e3, 4)})
    m.timing(False)

    # One buffer for every kernel of the step that stamps once g_rc_stamps is set: the tiled GEMMs
    # write 64 entries per workgroup from entry 0 (gemm.h; the largest grid of 128-row tiles at
    # batch 256 is 394 x 24 = 9 456 workgroups, 605 184 entries < STAMP_BASE), the fused kernel 16
    # per workgroup from QA_STAMP_BASE (qkv_attention.h).
    STAMP_BASE, per_wg = 1 << 20, 16
    nwg = 8 * 3 * ((args.batch + 1) // 2)
    assert args.batch * 197 // 128 * 24 * 64 < STAMP_BASE
    stamps = torch.zeros(STAMP_BASE + nwg * per_wg, dtype=torch.int64, device=dev)
    for v in [int(x) for x in args.phase_variants.split(",")]:
        m.set_qkv_sched(v + 8)
        run()
        stamps.zero_()
        L.check(raw_lib.rc_diag_set_stamps(C.c_void_p(stamps.data_ptr())))
        run()  # the stamps left are those of the last fused layer's launch
        L.check(raw_lib.rc_diag_set_stamps(None))
        st = stamps[STAMP_BASE:].cpu().numpy().reshape(-1, per_wg)
        st = st[st[:, 0] != 0]
        t0, t1, t2, t3 = st[:, 0], st[:, 1], st[:, 2], st[:, 3]
        wend = st[:, 4:8]
        tend = wend.max(axis=1)
        med = lambda x: round(float(np.median(x)) * TICK_US, 2)  # noqa: E731
        cus = len({(int(x) >> 32, (int(x) >> 8) & 0xFF, (int(x) >> 13) & 0x7) for x in st[:, 8]})
        emit({"kind": "phases", "variant": v, "blocks": int(len(st)), "cus": cus,
              "span_us": round(float(tend.max() - t0.min()) * TICK_US, 2),
              "prologue_us": med(t1 - t0), "kloop_us": med(t2 - t1), "epilogue_us": med(t3 - t2),
              "attention_us": med(tend - t3), "block_us": med(tend - t0),
              "wave_attention_us": [med(wend[:, w] - t3) for w in range(4)]})
    m.close()


if __name__ == "__main__":
    main()
