"""GPU tests of the mask inside the filter GEMM (``RC_SEARCH_MFMA_MASKED``, ``mode="mfma_masked"``):
the MASKED forms of the filter kernels against the masked scan, bit for bit.

Shapes.  n = 20001 rows, 16 queries, k = 10: the stage ratio is 64, so the stages are [0, 4096) and
[4096, 20001); the last row tile is ragged and the last bitmap word (rows 20000 .. 20031) lies
mostly past ``n_rows``.  The bitmaps hold exactly ceil(n / 32) words.
"""
import numpy as np
import pytest

from conftest import import_pkg
from test_masked_search_gpu import _check_vs_oracle, data, dev_mask, pack, same_bits, search_masked

pytestmark = pytest.mark.gpu

F8 = "float8_e4m3fn"
N, NQ, K = 20001, 16, 10


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


@pytest.fixture(scope="module")
def L(cuda):
    return import_pkg("_lib")


def build(idxmod, cuda, X, dtype, flt=None, metric="cosine"):
    import torch

    dev = idxmod.DeviceIndex(X.shape[1], dtype=dtype, capacity=X.shape[0] + 3, device=cuda, metric=metric)
    dev.upsert_rows(torch.from_numpy(X), torch.arange(X.shape[0], dtype=torch.int64))
    if flt is not None:
        dev.set_filter(flt)
    return dev


def masks(n):
    """name -> (flags, what to assert about the queries that fall back: None, "none" or "some")"""
    rng = np.random.default_rng(101)
    rows = np.arange(n)
    out = {f"random {share}": (rng.random(n) < share, None) for share in (0.5, 0.1, 0.01)}
    out["all ones"] = (np.ones(n, bool), None)
    # stage 1 sees no eligible row; stage 2 holds 3,617 eligible rows <= 4096 slots against thr = -inf
    out["rows >= 16384"] = (rows >= 16384, "none")
    # stage 2 holds 15,905 eligible rows against thr = -inf: every query overflows, and stays exact
    out["rows >= 4096"] = (rows >= 4096, "some")
    out["last row only"] = (rows == n - 1, None)
    out["3 rows"] = (np.isin(rows, [7, 4100, n - 2]), None)
    return out


# (dtype, dim, filter, metric): the filter_qs forms NKT 2 / 4 / 8, the generic filter_gemm_kernel (dim 192), the int8
# copy (RT 128 and 64; one on an f32 index), float8 (QT 2 and 1) and the METRIC forms of both native kernels
CONFIGS = [(dt, dim, None, "cosine") for dt in ("float16", "bfloat16") for dim in (128, 256, 512)] + [
    ("float16", 192, None, "cosine"),
    ("float16", 256, "i8", "cosine"),
    ("float32", 768, "i8", "cosine"),
    (F8, 256, "f8", "cosine"),
    (F8, 768, "f8", "cosine"),
    ("float16", 192, "metric", "dotproduct"),
    ("bfloat16", 512, "metric", "euclidean"),
]


@pytest.mark.parametrize("dtype,dim,flt,metric", CONFIGS)
def test_masked_filter_equals_the_masked_scan(idxmod, L, cuda, dtype, dim, flt, metric):
    import torch

    X, Q = data(N, dim, NQ, 97)
    if metric != "cosine":  # norms that matter to the metric
        X = X * np.random.default_rng(5).uniform(0.5, 2.0, (N, 1)).astype(np.float32)
    dev = build(idxmod, cuda, X, dtype, flt, metric)
    q = torch.from_numpy(Q)
    for name, (flags, fb) in masks(N).items():
        m = dev_mask(pack(flags), dev.device)
        assert m.numel() == (N + 31) // 32
        s0, r0 = search_masked(L, dev, q, K, N, m, mode="scan")
        dev.gemm_timing_read()
        s1, r1 = search_masked(L, dev, q, K, N, m, mode="mfma_masked")
        fallbacks = dev.gemm_timing_read()[3]
        assert same_bits(s0, s1) and np.array_equal(r0, r1), name
        kk = min(K, int(flags.sum()))
        assert np.all(flags[r1[:, :kk]]) and np.all(r1[:, kk:] == -1) and np.all(np.isneginf(s1[:, kk:])), name
        if fb == "none":
            assert fallbacks == 0, (name, fallbacks)
        if fb == "some":
            assert fallbacks > 0, name
        if name == "all ones":  # the unmasked batched search
            s2, r2 = search_masked(L, dev, q, K, N, None, mode="mfma")
            assert same_bits(s1, s2) and np.array_equal(r1, r2)
            s3, r3 = search_masked(L, dev, q, K, N, None, mode="mfma_masked")  # no mask: "mfma" itself
            assert same_bits(s1, s3) and np.array_equal(r1, r3)
        if name == "random 0.1":
            if metric == "cosine":
                _check_vs_oracle(dev.stored_rows(N).cpu().numpy(), Q, flags, K, s1, r1)
            # bits set past n_rows in the last word (rows 20001 .. 20031) change nothing
            words = pack(flags).copy()
            words[-1] |= np.uint32(0xFFFFFFFE)
            s4, r4 = search_masked(L, dev, q, K, N, dev_mask(words, dev.device), mode="mfma_masked")
            assert same_bits(s1, s4) and np.array_equal(r1, r4)
    dev.close()


def test_the_cliff_is_gone(idxmod, L, cuda):
    """65,536 x 128 f16, 16 queries, k = 100: the stage ratio is 16, the stages [0, 4096) and
    [4096, 65536).  Under a random mask the most eligible candidates any query collects in stage 2
    (numpy on the stored rows, threshold = the 100th eligible score of stage 1 minus 1e-3, three
    seeds) is 1,851 at share 0.25, 1,942 at 0.1 and 625 at 0.01 (there thr is still -inf: every
    eligible row), all below the 4096 slots: no query may fall back.  Without the mask in the filter
    the fewest any query collects is 5,073 at 0.25 and 11,755 at 0.1: "mfma" overflows for certain."""
    import torch

    n, dim, nq, k = 65536, 128, 16, 100
    X, Q = data(n, dim, nq, 83)
    dev = build(idxmod, cuda, X, "float16")
    q = torch.from_numpy(Q)
    rng = np.random.default_rng(89)
    for share in (0.25, 0.1, 0.01):
        flags = rng.random(n) < share
        m = dev_mask(pack(flags), dev.device)
        s0, r0 = search_masked(L, dev, q, k, n, m, mode="scan")
        dev.gemm_timing_read()
        s1, r1 = search_masked(L, dev, q, k, n, m, mode="mfma_masked")
        fallbacks = dev.gemm_timing_read()[3]
        assert same_bits(s0, s1) and np.array_equal(r0, r1), share
        assert fallbacks == 0, (share, fallbacks)
        if share == 0.1:  # the same mask at rescoring only: the candidate lists overflow
            s2, r2 = search_masked(L, dev, q, k, n, m, mode="mfma")
            assert dev.gemm_timing_read()[3] > 0
            assert same_bits(s0, s2) and np.array_equal(r0, r2)
    dev.close()


@pytest.mark.parametrize("remote", [False, True])
def test_sharded_equals_one_index(idxmod, L, cuda, remote):
    import torch

    n, dim, nq, k = 30000, 128, 16, 10
    X, Q = data(n, dim, nq, 61)
    ss = idxmod.ShardSet(dim, dtype="float16", capacity_per_shard=10240, devices=[0, 0, 0])
    if remote:
        ss.force_remote()
    ss.upsert_rows(torch.from_numpy(X), torch.arange(n))
    one = build(idxmod, cuda, X, "float16")
    q = torch.from_numpy(Q)
    flags = np.random.default_rng(67).random(n) < 0.1
    bm = pack(flags)
    s_ref, r_ref = search_masked(L, one, q, k, n, dev_mask(bm, one.device), mode="mfma_masked")
    s, r = ss.search(q, k, n, mode="mfma_masked", mask=bm)
    torch.cuda.synchronize()
    assert same_bits(s_ref, s.cpu().numpy()) and np.array_equal(r_ref, r.cpu().numpy())
    assert np.all(flags[r_ref])
    one.close()
    ss.close()


# --------------------------------------------------------------- Index level --
def test_query_batch_mode_and_auto_rule(idxmod, cuda):
    """``mode="mfma_masked"`` equals ``mode="scan"``; ``"auto"`` runs what ``_masked_mode`` says
    (filter launches exactly when it names a batched mode), the rule names "mfma_masked" for at least
    one of the cases, and 8 queries at share 0.25 over 65,536 rows still scan."""
    import torch

    n, dim = 65536, 128
    X, Q = data(n, dim, 64, 81)
    ix = idxmod.Index("mask-filter-auto", dimension=dim, dtype="float16", capacity=n, device=cuda)
    ix.upsert_tensor([f"v{i}" for i in range(n)], torch.from_numpy(X).to(cuda), [{"g": i % 100} for i in range(n)])
    dev = ix.shard_set.shard(0)
    dev.timing(True)
    assert ix._masked_mode("auto", 8, n, n // 4, 10) == "scan"
    assert ix._masked_mode("mfma_masked", 8, n, n // 4, 10) == "mfma_masked"  # a named mode is kept
    # the rule's other edges (a pure function of queries, rows per shard, share and k)
    assert ix._masked_mode("auto", 16, n, n // 10, 100) == "scan"  # under MASK_FILTER_MIN_QUERIES
    assert ix._masked_mode("auto", 64, n, n // 2, 100) == "mfma"  # MASKED_MFMA_MIN_SHARE keeps its rule
    assert ix._masked_mode("auto", 64, 1 << 20, 100, 100) == "scan"  # share 1e-4: below anything measured
    big = 16_000_000
    assert ix._masked_mode("auto", 32, big, big // 100, 10) == "scan"  # selective mask over many rows: the scan skips
    assert ix._masked_mode("auto", 32, big, big // 10, 10) == "mfma_masked"
    assert ix._masked_mode("auto", 256, big, big // 1000, 10) == "mfma_masked"
    assert ix._masked_mode("auto", 256, 2 * big, big // 5, 10) == "scan"  # larger shards were not measured
    picked = []
    for nq, k, flt, eligible in ((16, 10, {"g": {"$lt": 10}}, n // 100 * 10 + min(n % 100, 10)),
                                 (64, 100, {"g": {"$lt": 10}}, n // 100 * 10 + min(n % 100, 10)),
                                 (64, 100, {"g": 7}, n // 100 + (1 if n % 100 > 7 else 0)),
                                 (8, 10, {"g": {"$lt": 25}}, n // 100 * 25 + min(n % 100, 25))):
        q = torch.from_numpy(Q[:nq])
        want = ix._masked_mode("auto", nq, n, eligible, k)
        picked.append(want)
        ref = ix.query_batch(q, top_k=k, filter=flt, mode="scan")
        assert ix.query_batch(q, top_k=k, filter=flt, mode="mfma_masked") == ref
        dev.gemm_timing_read()
        got = ix.query_batch(q, top_k=k, filter=flt)
        launches = dev.gemm_timing_read()[1]
        assert got == ref
        assert (launches > 0) == (want in ("mfma", "mfma_masked")), (nq, k, flt, want, launches)
        assert all(len(r["matches"]) == k for r in got)
    assert picked[-1] == "scan"  # 8 queries
    assert "mfma_masked" in picked, picked
    ix.close()


# ------------------------------------------------------------------ refusals --
def test_refused_where_mfma_is(idxmod, cuda):
    import torch

    n, dim = 300, 256
    X, Q = data(n, dim, 4, 71)
    q = torch.from_numpy(Q)
    ones = dev_mask(np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32), cuda)
    cases = [("float32", None, "cosine"), (F8, None, "cosine"), ("float16", None, "dotproduct")]
    for dtype, flt, metric in cases:
        dev = build(idxmod, cuda, X, dtype, flt, metric)
        for mask in (None, ones):
            errs = []
            for mode in ("mfma", "mfma_masked"):
                with pytest.raises(ValueError) as e:
                    dev.search(q, 5, n, mode=mode, mask=mask)
                errs.append(str(e.value))
            assert errs[0] == errs[1]
        with pytest.raises(ValueError):
            dev.search(q, 5, n, mode="mfma_masked_too", mask=ones)
        dev.close()
