"""GPU tests of the float8 filter (rc_index_set_filter(RC_FILTER_F8)): the batched search of a
float8 index on the block-scaled fp8 MFMA.

Reference path replaced: Pinecone ``index.query`` (``retriever/utils.py:59-66``) for a batch of
query vectors, as in tests/test_batched_search_gpu.py.  Two bars.  The filter's own scores
(``DeviceIndex.filter_scores``) are compared with float64 dots of tests/f8_filter_model.py's CPU
model — with exact data, where a wrong operand byte order, LDS swizzle or scale byte shows as a
wrong number at 300 rows, and with Gaussian data, where the documented bound ``eps`` and the
accumulation bound ``c_acc`` (an assumption about the MFMA's internal sums) are measured.  And the
search: ``mode="mfma"`` returns EXACTLY (rows and score bits) what ``mode="scan"`` returns, with no
fallback on random rows — a filter that kept everything would still be exact through the fallback
scan, so the fallback count is part of the condition.

Measured on MI355X (largest |s' − (q_hi + q_lo)·x̂| / c_acc over the cases of
test_scores_low_term): see DESIGN.md § float8 filter.
"""
import numpy as np
import pytest

import f8_filter_model as fm
from conftest import import_pkg

pytestmark = pytest.mark.gpu

F8 = "float8_e4m3fn"


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


def _f8_index(idxmod, cuda, X, dim, capacity=None):
    import torch

    X = X if isinstance(X, torch.Tensor) else torch.from_numpy(X)
    n = X.shape[0]
    dev = idxmod.DeviceIndex(dim, dtype=F8, capacity=capacity or n, device=cuda)
    dev.upsert_rows(X, torch.arange(n, dtype=torch.int64))
    dev.set_filter("f8")
    assert dev.filter == "f8"
    return dev


def _same(dev, Q, k, n, mask=None):
    import torch

    s_m, r_m = dev.search(Q, k, n, mode="mfma", mask=mask)
    s_s, r_s = dev.search(Q, k, n, mode="scan", mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(r_m, r_s), "float8-filtered batched search and scan disagree on rows"
    assert torch.equal(s_m, s_s), "float8-filtered batched search and scan disagree on score bits"
    return s_m, r_m


def _gpu_unit(idxmod, cuda, Q):
    """The library's own f32 normalisation of Q: what prepare_queries_f8_kernel splits."""
    import torch

    f32 = idxmod.DeviceIndex(Q.shape[1], dtype="float32", capacity=Q.shape[0], device=cuda)
    f32.upsert_rows(torch.from_numpy(Q), torch.arange(Q.shape[0], dtype=torch.int64))
    out = f32.stored_rows(Q.shape[0]).cpu().numpy()
    f32.close()
    return out


# ------------------------------------------------------------------ 1. scores, exact data
@pytest.mark.parametrize("dim", [512, 768])
def test_scores_exact_data(idxmod, cuda, dim):
    import torch

    n, nq = 300, 20
    X, Q = fm.exact_rows_and_queries(dim, n, nq)
    dev = _f8_index(idxmod, cuda, X, dim)
    stored = dev.stored_rows(n).cpu().numpy()
    assert (stored == fm.unit_f32(X)).all()  # exactly representable: nothing was rounded
    want = fm.dot64(fm.unit_f32(Q), stored)
    tol = fm.c_acc(fm.ld_of(dim))
    for row0, cnt in ((0, 300), (128, 172)):  # two tile boundaries and a partial tile; a later first row
        s, eps = dev.filter_scores(torch.from_numpy(Q), row0, cnt)
        torch.cuda.synchronize()
        s = s.cpu().numpy().astype(np.float64)
        err = np.abs(s - want[:, row0:row0 + cnt]).max()
        print(f"exact data dim {dim} rows [{row0}, {row0 + cnt}): max |s' - dot| = {err:.3e} (c_acc {tol:.3e})")
        assert s.shape == (nq, cnt)
        assert err <= tol
        assert (eps.cpu().numpy() >= tol).all()
    dev.close()


# ------------------------------------------------------------------ 2. scores, low term
@pytest.mark.parametrize("dim", [100, 512, 768])
def test_scores_low_term(idxmod, cuda, dim):
    import torch

    n, nq = 300, 20
    rng = np.random.default_rng(dim)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    dev = _f8_index(idxmod, cuda, X, dim)
    stored = dev.stored_rows(n).cpu().numpy()
    qhat = _gpu_unit(idxmod, cuda, Q)
    hi, lo, _, _ = fm.split(qhat)
    tol = fm.c_acc(fm.ld_of(dim))
    low = np.abs(fm.dot64(lo, stored))
    assert low.max() > 10 * tol  # precondition: a kernel that dropped or mis-scaled q_lo is off by more than the bound
    s, eps = dev.filter_scores(torch.from_numpy(Q), 0, n)
    torch.cuda.synchronize()
    s = s.cpu().numpy().astype(np.float64)
    eps = eps.cpu().numpy().astype(np.float64)
    err_true = np.abs(s - fm.dot64(qhat, stored))
    err_model = np.abs(s - (fm.dot64(hi, stored) + fm.dot64(lo, stored)))
    print(f"dim {dim}: max |s' - q.x| / eps = {(err_true / eps[:, None]).max():.3f}; "
          f"max |s' - (q_hi + q_lo).x| = {err_model.max():.3e} = {err_model.max() / tol:.4f} c_acc; eps mean {eps.mean():.2e}")
    assert (err_true <= eps[:, None]).all()
    assert err_model.max() <= tol
    assert eps.max() < 2e-3  # two terms: the f16 filter's order, no stage inflation needed
    dev.close()


# ------------------------------------------------------------------ 3. search parity
@pytest.mark.parametrize("dim", [512, 768, 100])
@pytest.mark.parametrize("n,k,nq", [(200, 5, 3), (5000, 10, 9), (70_000, 100, 20), (70_000, 256, 9), (300_000, 10, 300)])
def test_f8_filter_matches_scan(idxmod, cuda, dim, n, k, nq):
    import torch

    g = torch.Generator(device="cuda").manual_seed(n + dim + k + nq)
    X = torch.randn((n, dim), device="cuda", generator=g)
    Q = torch.randn((nq, dim), device="cuda", generator=g)
    Q[0] = X[n // 3]
    dev = _f8_index(idxmod, cuda, X, dim)
    dev.timing(True)
    dev.gemm_timing_read()
    s_m, r_m = dev.search(Q, k, n, mode="mfma")
    _, launches, _, fallbacks = dev.gemm_timing_read()
    dev.timing(False)
    s_s, r_s = dev.search(Q, k, n, mode="scan")
    torch.cuda.synchronize()
    assert torch.equal(r_m, r_s) and torch.equal(s_m, s_s)
    assert int(r_m[0, 0]) == n // 3
    assert fallbacks == 0  # random rows: the filter itself kept the lists short
    # the filter kernel ran (the first stage's launch keeps every row: its threshold is -inf; from
    # n = 5000 on a later stage filters against a real one)
    assert launches > (1 if n > 4096 else 0)
    dev.close()


# ------------------------------------------------------------------ 4. rows aligned with the rounding residual
def test_rows_along_the_query_rounding_residual(idxmod, cuda):
    import torch

    dim, n, nq, k, n_first = 512, 70_000, 16, 20, 4096
    X, Q, rows_a, rows_b = fm.planted_case(dim, n, nq, k, n_first)
    dev = _f8_index(idxmod, cuda, X, dim)
    stored = dev.stored_rows(n).cpu().numpy()
    qhat = _gpu_unit(idxmod, cuda, Q)
    hi, _, _, _ = fm.split(qhat)
    _, eps = dev.filter_scores(torch.from_numpy(Q), 0, 128)
    eps = eps.cpu().numpy().astype(np.float64)
    true = fm.dot64(qhat, stored)
    one = fm.dot64(hi, stored)
    dropped = 0
    for q in range(nq):
        order = np.argsort(-true[q])
        assert set(order[:k]) == set(rows_a[q])
        assert true[q][order[k - 1]] - true[q][order[k]] > 2 * eps[q]
        thr = np.sort(true[q][:n_first])[-k] - eps[q]  # the threshold after the first stage
        dropped += int((one[q][rows_a[q]] < thr).sum())
    assert dropped >= 1, "precondition: a one-term filter with the two-term eps would drop a planted row"
    _, r = _same(dev, torch.from_numpy(Q), k, n)
    assert [set(x) for x in r.cpu().tolist()] == [set(x) for x in rows_a.tolist()]
    dev.close()


# ------------------------------------------------------------------ 5. duplicates
def test_duplicates_fall_back_exactly(idxmod, cuda):
    import torch

    dim, n, k = 512, 70_000, 10
    g = torch.Generator(device="cuda").manual_seed(5)
    X = torch.randn((n, dim), device="cuda", generator=g)
    X[10_000:16_000] = X[9_999]  # 6000 copies past the first stage: more than the candidate lists hold
    Q = torch.randn((16, dim), device="cuda", generator=g)
    Q[0] = X[9_999]
    dev = _f8_index(idxmod, cuda, X, dim)
    dev.timing(True)
    dev.gemm_timing_read()
    s_m, r_m = dev.search(Q, k, n, mode="mfma")
    fallbacks = dev.gemm_timing_read()[3]
    dev.timing(False)
    s_s, r_s = dev.search(Q, k, n, mode="scan")
    assert torch.equal(r_m, r_s) and torch.equal(s_m, s_s)
    assert fallbacks > 0
    assert r_m[0].cpu().tolist() == list(range(9_999, 9_999 + k))  # ties by ascending row
    dev.close()


# ------------------------------------------------------------------ 6. mask
@pytest.mark.parametrize("share", [0.6, 0.01])
def test_masked_mfma_matches_masked_scan(idxmod, cuda, share):
    import torch

    dim, n, nq, k = 256, 70_000, 16, 10
    g = torch.Generator(device="cuda").manual_seed(6)
    X = torch.randn((n, dim), device="cuda", generator=g)
    Q = torch.randn((nq, dim), device="cuda", generator=g)
    rng = np.random.default_rng(int(share * 100))
    bits = rng.random(n) < share
    words = np.packbits(np.pad(bits, (0, -n % 32)).reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).ravel()
    mask = torch.from_numpy(words.view(np.int32).copy()).cuda()
    dev = _f8_index(idxmod, cuda, X, dim)
    _, r = _same(dev, Q, k, n, mask=mask)
    assert bits[r.cpu().numpy().ravel()].all()
    dev.close()


# ------------------------------------------------------------------ 7. auto
def test_auto_takes_the_filter_under_its_conditions(idxmod, cuda):
    """The "f8" kind's own "auto" corner, measured (index.hip, kF8BatchMinPasses): the filter from 16
    scan passes (64 queries at this width: 4 per pass) over 131 072 rows, or from 8 passes over
    2^28 bytes of rows.  16 queries x 70 000 rows, the corner of the f16 filter, scans: there the
    float8 scan was faster."""
    import torch

    dim, n = 256, 1_100_000
    dev = idxmod.DeviceIndex(dim, dtype=F8, capacity=n, device=cuda)
    dev.fill_random(7, 0, n)
    dev.set_filter("f8")
    g = torch.Generator(device="cuda").manual_seed(7)
    Q = torch.randn((64, dim), device="cuda", generator=g)
    dev.timing(True)
    cases = ((64, 140_000, True), (60, 140_000, False), (64, 120_000, False), (16, 70_000, False),
             (32, 1_050_000, True), (28, 1_050_000, False), (32, 1_000_000, False))
    for nq, rows, expect in cases:
        dev.gemm_timing_read()
        s_a, r_a = dev.search(Q[:nq], 10, rows, mode="auto")
        launches = dev.gemm_timing_read()[1]
        s_s, r_s = dev.search(Q[:nq], 10, rows, mode="scan")
        assert torch.equal(r_a, r_s) and torch.equal(s_a, s_s)
        assert (launches > 0) == expect, (nq, rows, launches)
    dev.timing(False)
    dev.close()


# ------------------------------------------------------------------ 8. shards and the Pinecone layer
def test_shard_set(idxmod, cuda):
    import torch

    dim, n, k = 256, 30_000, 10
    g = torch.Generator(device="cuda").manual_seed(8)
    X = torch.randn((n, dim), device="cuda", generator=g)
    Q = torch.randn((16, dim), device="cuda", generator=g)
    for remote in (False, True):
        sset = idxmod.ShardSet(dim, dtype=F8, capacity_per_shard=n // 3, devices=[cuda, cuda, cuda])
        if remote:
            sset.force_remote()
        sset.upsert_rows(X, torch.arange(n, dtype=torch.int64))
        sset.set_filter("f8")
        assert sset.filter == "f8" and all(sset.shard(s).filter == "f8" for s in range(3))
        s1, r1 = sset.search(Q, k, n, mode="mfma")
        s2, r2 = sset.search(Q, k, n, mode="scan")
        assert torch.equal(r1, r2) and torch.equal(s1, s2)
        sset.close()


def _matches(res):
    return [[(m["id"], m["score"]) for m in r["matches"]] for r in res]


def test_pinecone_layer(idxmod, cuda, tmp_path):
    import torch

    dim, n = 256, 70_000
    g = torch.Generator(device="cuda").manual_seed(9)
    X = torch.randn((n, dim), device="cuda", generator=g)
    Q = torch.randn((16, dim), device="cuda", generator=g).cpu()
    ids = [f"v{i}" for i in range(n)]
    f8 = idxmod.Index("x", dimension=dim, dtype="f8", filter="f8", capacity=n, device=cuda)
    nat = idxmod.Index("x", dimension=dim, dtype="f8", filter="native", capacity=n, device=cuda)
    for ix in (f8, nat):
        ix.upsert_tensor(ids, X)
    dev = f8.shard_set.shard(0)
    dev.timing(True)
    dev.gemm_timing_read()
    got = _matches(f8.query_batch(Q, top_k=10, mode="mfma"))
    assert dev.gemm_timing_read()[1] > 0  # the filter ran
    dev.timing(False)
    assert got == _matches(nat.query_batch(Q, top_k=10))
    assert got == _matches(f8.query_batch(Q, top_k=10))  # "auto", whichever path it takes
    assert f8._masked_mode("auto", 64, 1 << 20, 1 << 20) == "mfma" and nat._masked_mode("auto", 64, 1 << 20, 1 << 20) == "scan"
    assert f8._masked_mode("auto", 16, 70_000, 70_000) == "scan"  # below the kind's own corner
    f8.save(str(tmp_path / "snap"))
    back = idxmod.Index.load(str(tmp_path / "snap"), device=cuda)
    assert back.shard_set.filter == "f8"
    assert _matches(back.query_batch(Q, top_k=10, mode="mfma")) == got
    back.close()
    gone = [f"v{i}" for i in range(0, 3000, 3)]  # 1000 ids: rows move in from the end
    for ix in (f8, nat):
        ix.delete(ids=gone)
    after = _matches(f8.query_batch(Q, top_k=10, mode="mfma"))
    assert after == _matches(nat.query_batch(Q, top_k=10, mode="scan"))
    assert not {i for m in after for i, _ in m} & set(gone)
    f8.close()
    nat.close()


# ------------------------------------------------------------------ 9. refusals
def test_refusals(idxmod, cuda):
    import torch

    f16 = idxmod.DeviceIndex(256, dtype="float16", capacity=64, device=cuda)
    with pytest.raises(ValueError):
        f16.set_filter("f8")
    assert f16.filter == "native"
    f16.close()
    wide = idxmod.DeviceIndex(1000, dtype=F8, capacity=64, device=cuda)  # ld 1024
    with pytest.raises(ValueError):
        wide.set_filter("f8")
    wide.close()
    dot = idxmod.DeviceIndex(256, dtype=F8, capacity=64, device=cuda)
    dot.set_metric("dotproduct")
    with pytest.raises(ValueError):
        dot.set_filter("f8")
    assert dot.filter == "native"
    dot.close()

    dev = idxmod.DeviceIndex(256, dtype=F8, capacity=64, device=cuda)
    dev.fill_random(1, 0, 64)
    q = torch.randn((8, 256))
    with pytest.raises(ValueError):
        dev.filter_scores(q, 0, 64)  # "native": no float8 filter to look into
    with pytest.raises(ValueError):
        dev.search(q, 5, 64, mode="mfma")
    dev.set_filter("f8")
    with pytest.raises(ValueError):
        dev.set_filter("i8")  # stays refused on a float8 index
    assert dev.filter == "f8"
    with pytest.raises(ValueError):
        dev.set_metric("euclidean")
    assert dev.metric == "cosine" and dev.filter == "f8"
    with pytest.raises(ValueError):
        dev.filter_scores(q, 64, 0 + 1)  # row0 + n beyond the capacity
    s_m, r_m = dev.search(q, 5, 64, mode="mfma")
    s_s, r_s = dev.search(q, 5, 64, mode="scan")
    assert torch.equal(r_m, r_s) and torch.equal(s_m, s_s)
    dev.set_filter("native")
    assert dev.filter == "native"
    with pytest.raises(ValueError):
        dev.search(q, 5, 64, mode="mfma")
    dev.set_metric("euclidean")  # legal again
    dev.close()

    sset = idxmod.ShardSet(256, dtype=F8, capacity_per_shard=64, devices=[cuda, cuda])
    sset.set_filter("f8")
    with pytest.raises(ValueError):
        sset.set_metric("euclidean")
    assert sset.metric == "cosine" and sset.filter == "f8"
    assert all(sset.shard(s).metric == "cosine" and sset.shard(s).filter == "f8" for s in range(2))
    sset.close()
