"""What v_mfma_scale_f32_16x16x128_f8f6f4 does with its operands, measured through rc_gemm_mxfp8 (GPU).

    python tools/mx_mfma_probe.py        # log: profiles/mxfp8/mfma_probe.log

1. Layout: data 1.0 in one 16-byte chunk c of K = 128, one scale block j set to 8x: which (c, j) pairs
   multiply?  (16 = the chunk unscaled, 128 = scaled.)
2. Accumulation: one product of 1.0 beside n products of t * 2^-s (their blocks' scale).  Exact sum
   1 + n t 2^-s; printed is (out - 1) * 2^s / (n t), 1 while the small products survive.  An f32 chain
   rounding to nearest keeps them to s = 24 + log2(n t) or so; a sum that aligns every product to the
   largest exponent and keeps w bits below it drops each of them once s > w.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import import_pkg  # noqa: E402

L = import_pkg("_lib")
lib = L.load()
ONE, ONE75 = 0x38, 0x3E  # e4m3 1.0 and 1.75


def run(A8, As, W8, Ws):
    M, K = A8.shape
    A8, As, W8, Ws = (x.cuda() for x in (A8, As, W8, Ws))  # held until the synchronize below
    bias = torch.zeros(768, device="cuda")
    out = torch.zeros(M, 768, device="cuda")
    L.check(lib.rc_gemm_mxfp8(A8.data_ptr(), As.data_ptr(), W8.data_ptr(), Ws.data_ptr(), bias.data_ptr(), M, 768, K,
                              out.data_ptr(), 197, None))
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64)


def ones(rows, K, byte=ONE, scale=127):
    return torch.full((rows, K), byte, dtype=torch.uint8), torch.full((rows, K // 32), scale, dtype=torch.uint8)


def layout(vary_a):
    X8, Xs = torch.zeros(32, 128, dtype=torch.uint8), torch.full((32, 4), 127, dtype=torch.uint8)
    for c in range(8):
        for j in range(4):
            X8[c * 4 + j, 16 * c:16 * c + 16] = ONE
            Xs[c * 4 + j, j] = 130
    if vary_a:
        o = run(X8, Xs, *ones(768, 128))[:, 5]
    else:
        W8, Ws = ones(768, 128, 0)
        W8[:32], Ws[:32] = X8, Xs
        o = run(*ones(40, 128), W8, Ws)[7, :32]
    print("layout, varying", "A" if vary_a else "W", "(rows: chunk c, columns: scale block j)")
    print(o.reshape(8, 4))


def accumulation(K, byte, t):
    S = list(range(14, 36))
    A8, As = torch.zeros(len(S), K, dtype=torch.uint8), torch.full((len(S), K // 32), 127, dtype=torch.uint8)
    A8[:, 0] = ONE
    A8[:, 32:] = byte  # K = 128: blocks 1-3 of the same instruction; K = 256: also the whole second one
    for r, s in enumerate(S):
        As[r, 1:] = 127 - s
    o = run(A8, As, *ones(768, K))[:, 0]
    n = K - 32
    print(f"accumulation, K = {K}, {n} products of {t} * 2^-s beside 1.0: s, (out - 1) * 2^s / ({n} * {t})")
    print("  ".join(f"{s}:{(o[r] - 1) * 2.0 ** s / (n * t):.4f}" for r, s in enumerate(S)))


def subnormals():
    # e4m3 subnormals m * 2^-9 (bytes 0x01 .. 0x07) as A against 1.0, and as W against 1.0: 128 m 2^-9
    for side in "AW":
        got = []
        for mant in (1, 3, 7):
            sub, one = ones(768 if side == "W" else 16, 128, mant), ones(16 if side == "W" else 768, 128)
            got.append(run(*sub, *one)[0, 0] if side == "A" else run(*one, *sub)[0, 0])
        print(f"subnormal {side} bytes 1, 3, 7 against 1.0 over K = 128: expect 0.25 0.75 1.75, got", *got)


subnormals()
layout(True)
layout(False)
accumulation(128, ONE, 1.0)
accumulation(128, ONE75, 1.75)
accumulation(256, ONE, 1.0)
