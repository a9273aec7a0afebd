"""A CPU model of the float8 filter's arithmetic (csrc/search_mfma.hip, RC_FILTER_F8), shared by
tests/test_f8_filter_cpu.py and tests/test_f8_filter_gpu.py.  torch's ``float8_e4m3fn`` conversion
(round to nearest even, OCP e4m3fn) stands for ``v_cvt_pk_fp8_f32``; dots are float64.

    stored row   x̂ = e4m3(x · 2⁸) · 2⁻⁸            (x the f32 unit vector)
    q_hi          = e4m3(q̂ · 2⁸) · 2⁻⁸            (the same rule)
    q_lo          = e4m3((q̂ − q_hi) · 2¹²) · 2⁻¹²
    s'            = (q_hi + q_lo) · x̂
    |s' − q̂ · x̂| <= ‖q̂ − q_hi − q_lo‖ · ‖x̂‖  (Cauchy-Schwarz) + the accumulation bound c_acc
"""
import numpy as np
import torch

ROW_NORM_MAX = 1.07


def ld_of(dim: int) -> int:
    """Row width of a float8 index: dim rounded up to 256."""
    return (dim + 255) // 256 * 256


def c_acc(ld: int, terms: int = 2) -> float:
    """The filter's accumulation bound: 6.5e-5 for the exact score's f32 chain, plus a truncation
    (2⁻²³ relative, on partial sums below 1.07) at each of the ld + terms · ld/128 additions."""
    return 6.5e-5 + (ld + terms * (ld // 128)) * 2.0 ** -23 * ROW_NORM_MAX


def unit_f32(v: np.ndarray) -> np.ndarray:
    """Rows of v normalised as the library does it, up to the last bit: f32 in, f32 out."""
    v = np.asarray(v, dtype=np.float32)
    n = np.sqrt((v.astype(np.float64) ** 2).sum(axis=-1, keepdims=True)).astype(np.float32)
    return (v * (np.float32(1.0) / n)).astype(np.float32)


def e4m3(x: np.ndarray) -> np.ndarray:
    """x (f32) rounded to e4m3fn, as f32."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float8_e4m3fn).to(torch.float32).numpy()


def store(xhat: np.ndarray) -> np.ndarray:
    """The stored value of unit rows: e4m3(x̂ · 2⁸) · 2⁻⁸ (exact in f32)."""
    return e4m3(xhat * np.float32(256.0)) * np.float32(1.0 / 256.0)


def split(qhat: np.ndarray):
    """(q_hi, q_lo, the scaled low-term input (q̂ − q_hi) · 2¹², the residual q̂ − q_hi − q_lo), all f32."""
    qhat = np.asarray(qhat, dtype=np.float32)
    hi = store(qhat)
    d = (qhat - hi).astype(np.float32)
    lo_in = d * np.float32(4096.0)
    lo = e4m3(lo_in) * np.float32(1.0 / 4096.0)
    return hi, lo, lo_in, (d - lo).astype(np.float32)


def dot64(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return a.astype(np.float64) @ b.astype(np.float64).T


def exact_pattern(dim: int, seed: int) -> np.ndarray:
    """dim values in {0, ±1, ±2} with sum of squares exactly 1024: 224 of ±1, 200 of ±2.  A vector
    that is a permutation of them has norm 32, so its unit form has elements in {0, ±2⁻⁵, ±2⁻⁴}:
    exactly representable in e4m3 · 2⁻⁸, with a zero low term, and every dot of two such unit
    vectors is a multiple of 2⁻¹⁰ below 4, exact in f32 in any summation order."""
    rng = np.random.default_rng(seed)
    p = np.zeros(dim, dtype=np.float32)
    p[:224] = 1.0
    p[224:424] = 2.0
    p *= rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=dim)
    return p[rng.permutation(dim)]


def exact_rows_and_queries(dim: int, n: int, nq: int):
    """Row r holds pattern[(3r + 5c) mod dim] at column c, query q another pattern at (7q + c) mod dim:
    bijections of the columns (5 and 1 are coprime to 512 and 768), asymmetric in rows and queries,
    so that a swapped or permuted operand map cannot cancel."""
    assert dim % 5 != 0 and dim % 2 == 0
    pr, pq = exact_pattern(dim, 1), exact_pattern(dim, 2)
    c = np.arange(dim)
    X = np.stack([pr[(3 * r + 5 * c) % dim] for r in range(n)])
    Q = np.stack([pq[(7 * q + c) % dim] for q in range(nq)])
    return X, Q


def planted_case(dim: int, n: int, nq: int, k: int, n_first: int, seed: int = 4):
    """Rows aligned with the query rounding residual.  For each query: k rows A = normalise(cos θ · q̂ +
    sin θ · r̂), r̂ the unit rounding residual q̂ − q_hi (its part orthogonal to q̂), planted past row
    n_first; 200 rows B = normalise(cos φ · q̂ − sin φ · r̂)
    inside the first n_first rows, whose true score is a little below A's and whose q_hi-only score
    is above.  Returns (X f32 [n, dim], Q f32 [nq, dim], rows_a [nq, k], rows_b [nq, 200])."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    qhat = unit_f32(Q).astype(np.float64)
    hi = store(unit_f32(Q)).astype(np.float64)
    r = qhat - hi
    r -= (r * qhat).sum(axis=1, keepdims=True) * qhat  # the residual's part orthogonal to q̂: a row's true score is cos θ
    rhat = r / np.linalg.norm(r, axis=1, keepdims=True)
    theta = np.deg2rad(60.0)
    phi = np.arccos(np.cos(theta) - 13e-3)
    nb = 200
    assert nq * nb <= n_first and n_first + nq * k <= n
    rows_b = np.arange(nq * nb).reshape(nq, nb) * (n_first // (nq * nb))
    rows_a = n_first + 7 + np.arange(nq * k).reshape(nq, k) * ((n - n_first - 8) // (nq * k))
    for q in range(nq):
        jitter = 0.005 * unit_f32(rng.standard_normal((k + nb, dim))).astype(np.float64)
        X[rows_a[q]] = (np.cos(theta) * qhat[q] + np.sin(theta) * rhat[q] + jitter[:k]).astype(np.float32)
        X[rows_b[q]] = (np.cos(phi) * qhat[q] - np.sin(phi) * rhat[q] + jitter[k:]).astype(np.float32)
    return X, Q, rows_a, rows_b
