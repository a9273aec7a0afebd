"""The float8 filter (RC_FILTER_F8) without a GPU: the binding and the header know the new kind and
entry point, and a CPU model of the two-term e4m3 query split (tests/f8_filter_model.py) has the
properties the kernel's bound rests on: the low term's input never reaches e4m3's 448, two terms
leave a residual of the f16 filter's order, and the score error against float8-rounded rows is
within residual norm x row norm.
"""
import os
import re

import numpy as np
import pytest

import f8_filter_model as fm
from conftest import REPO, import_pkg

HEADER = os.path.join(REPO, "include", "retrieval_core.h")


def test_binding_and_header_know_the_f8_filter():
    L = import_pkg("_lib")
    assert L.FILTERS["f8"] == 2 and L.RC_FILTER_F8 == 2
    assert L.FILTERS["native"] == 0 and L.FILTERS["i8"] == 1
    src = open(HEADER).read()
    assert re.search(r"^#define\s+RC_FILTER_F8\s+2\s*$", src, flags=re.M)
    assert re.search(r"\bint\s+rc_index_filter_scores\s*\(", src)
    assert "rc_index_filter_scores" in L.SIGNATURES


def test_library_resolves_every_symbol_at_load():
    """Loaded with immediate binding: a kernel whose host-side stub the compiler dropped (it happens
    without a diagnostic inside templates) is an undefined symbol here, not at its first launch."""
    import ctypes

    ctypes.CDLL(import_pkg("_lib").LIB_PATH, mode=os.RTLD_NOW)


def test_index_constructor_pairs_filter_and_dtype():
    """Refused before any device call: "i8" on float8, "f8" on anything else, either on a non-cosine index."""
    idxmod = import_pkg("index")
    with pytest.raises(ValueError):
        idxmod.Index("x", dimension=64, dtype="f8", filter="i8")
    for dtype in ("float32", "float16", "bfloat16"):
        with pytest.raises(ValueError):
            idxmod.Index("x", dimension=64, dtype=dtype, filter="f8")
    with pytest.raises(ValueError):
        idxmod.Index("x", dimension=64, dtype="f8", filter="f8", metric="euclidean")


def _queries(kind: str, dim: int, n: int, rng) -> np.ndarray:
    if kind == "gauss":
        return rng.standard_normal((n, dim)).astype(np.float32)
    if kind == "one_hot":
        q = np.zeros((n, dim), dtype=np.float32)
        q[np.arange(n), rng.integers(0, dim, n)] = rng.choice(np.array([-3.0, 0.5], dtype=np.float32), n)
        return q
    if kind == "dominant":  # one dominant component, 1e-3 noise
        q = (1e-3 * rng.standard_normal((n, dim))).astype(np.float32)
        q[np.arange(n), rng.integers(0, dim, n)] = 1.0
        return q
    assert kind == "tiny"  # unit vectors with most components below 2^-14
    q = (2.0 ** -16 * rng.standard_normal((n, dim))).astype(np.float32)
    q[:, :4] = rng.standard_normal((n, 4)).astype(np.float32)
    return q


CASES = [("gauss", 100), ("gauss", 512), ("gauss", 768), ("one_hot", 512), ("dominant", 512), ("tiny", 768)]


@pytest.mark.parametrize("kind,dim", CASES)
def test_two_term_split(kind, dim):
    rng = np.random.default_rng(dim + len(kind))
    qhat = fm.unit_f32(_queries(kind, dim, 1024, rng))
    if kind == "tiny":
        assert (np.abs(qhat) < 2.0 ** -14).mean() > 0.9
    hi, lo, lo_in, resid = fm.split(qhat)
    # nothing saturates: |q̂_c − q_hi,c| <= 2⁻⁴ |q̂_c| <= 2⁻⁴, so the low term's input is below 256
    assert np.abs(lo_in).max() <= 448.0
    assert np.abs(qhat * np.float32(256.0)).max() <= 448.0
    rn = np.linalg.norm(resid.astype(np.float64), axis=1)
    one = np.linalg.norm((qhat - hi).astype(np.float64), axis=1)
    print(f"{kind} dim {dim}: one-term residual mean {one.mean():.2e} max {one.max():.2e}; "
          f"two-term mean {rn.mean():.2e} max {rn.max():.2e}")
    if kind == "gauss":
        assert rn.max() < 1.5e-3
        assert one.mean() > 10 * rn.mean()  # what the second term buys
    # the score error against float8-rounded rows is within residual norm x row norm
    xs = fm.store(fm.unit_f32(rng.standard_normal((300, dim)).astype(np.float32)))
    xn = np.linalg.norm(xs.astype(np.float64), axis=1)
    assert xn.max() <= fm.ROW_NORM_MAX and xn.min() >= 2.0 - fm.ROW_NORM_MAX
    exact = fm.dot64(qhat, xs)
    filt = fm.dot64(hi, xs) + fm.dot64(lo, xs)
    assert (np.abs(exact - filt) <= rn[:, None] * xn[None, :] + 1e-12).all()


def test_exact_data_has_no_low_term():
    """The exact-data case of the GPU score test: unit elements in {0, ±2⁻⁵, ±2⁻⁴}, q_lo = 0, and
    scores that are multiples of 2⁻¹⁰."""
    for dim in (512, 768):
        X, Q = fm.exact_rows_and_queries(dim, 40, 20)
        for v in (X, Q):
            u = fm.unit_f32(v)
            assert set(np.unique(np.abs(u))) <= {0.0, 2.0 ** -5, 2.0 ** -4}
            hi, lo, _, resid = fm.split(u)
            assert (hi == u).all() and (lo == 0).all() and (resid == 0).all()
            assert (fm.store(u) == u).all()
        s = fm.dot64(fm.unit_f32(Q), fm.unit_f32(X)) * 1024.0
        assert (s == np.round(s)).all() and len(np.unique(s)) > 20


def test_planted_case_defeats_a_one_term_filter():
    """The preconditions of the GPU test with rows along the rounding residual, on the CPU model's
    stored rows: the planted rows are the true top-k by more than 2·eps, and a one-term filter
    (q_hi only) with the two-term eps would drop one."""
    dim, n, nq, k, n_first = 512, 70_000, 16, 20, 4096
    X, Q, rows_a, rows_b = fm.planted_case(dim, n, nq, k, n_first)
    qhat = fm.unit_f32(Q)
    hi, lo, _, resid = fm.split(qhat)
    eps = fm.ROW_NORM_MAX * np.linalg.norm(resid.astype(np.float64), axis=1) * 1.001 + fm.c_acc(fm.ld_of(dim))
    xs = fm.store(fm.unit_f32(X))
    true = fm.dot64(qhat, xs)
    one = fm.dot64(hi, xs)
    dropped = 0
    for q in range(nq):
        order = np.argsort(-true[q])
        assert set(order[:k]) == set(rows_a[q])
        assert true[q][order[k - 1]] - true[q][order[k]] > 2 * eps[q]
        assert one[q][rows_b[q]].min() > one[q][rows_a[q]].max()  # the one-term scores rank B above A
        thr = np.sort(true[q][:n_first])[-k] - eps[q]  # after the first stage
        dropped += int((one[q][rows_a[q]] < thr).sum())
    assert dropped >= 1
