"""GPU tests of the float32 filter (RC_FILTER_F32): the batched MFMA search on the stored rows of a
float32 index under all three metrics.  Its filter GEMM rounds the rows to f16 (to nearest even) and
bounds the exact score; ``mode="mfma"`` must equal ``mode="scan"`` BIT FOR BIT, scores and rows.
Data, queries and the comparison are ``test_metric_filter_gpu``'s; the first stage takes the first
4096 rows unfiltered, so every shape has n > 4096 and whatever a test plants sits past row 4096.
"""
import numpy as np
import pytest

from conftest import import_pkg
from test_metric_filter_gpu import FIRST_STAGE, SHAPES, assert_same_bits, data, queries
from test_metrics_gpu import check_against_reference, reference

pytestmark = pytest.mark.gpu

METRICS = ["cosine", "dotproduct", "euclidean"]
# row widths 128, 512, 768 and (100: a padded row) 128 again; 256 on the smallest shape
CASES = [(d,) + s for d in (128, 512, 768, 100) for s in SHAPES] + [(256,) + SHAPES[0]]


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


def f32_index(idxmod, cuda, X, metric="cosine"):
    import torch

    dev = idxmod.DeviceIndex(X.shape[1], dtype="float32", capacity=X.shape[0], device=cuda, metric=metric)
    dev.upsert_rows(torch.from_numpy(X), torch.arange(X.shape[0]))
    dev.set_filter("f32")
    return dev


_DEVS = {}


@pytest.fixture(scope="module")
def devs(idxmod, cuda):
    """float32 DeviceIndex with the "f32" filter per (dim, n): built once, rows left unchanged."""
    def get(dim, n):
        if (dim, n) not in _DEVS:
            _DEVS[dim, n] = f32_index(idxmod, cuda, data(dim, n)[0])
        return _DEVS[dim, n]

    yield get
    for dev in _DEVS.values():
        dev.close()
    _DEVS.clear()


def batched_and_scan(dev, Q, k, n, mask=None, mode="mfma"):
    """(batched result, scan result, fallbacks of the batched search)"""
    dev.timing(True)
    dev.gemm_timing_read()
    got = dev.search(Q, k, n, mode=mode, mask=mask)
    fallbacks = dev.gemm_timing_read()[3]
    dev.timing(False)
    return got, dev.search(Q, k, n, mode="scan", mask=mask), fallbacks


# ------------------------------------------------------------------ 1. equals the scan
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim,n,k,nq", CASES)
def test_mfma_equals_scan(devs, dim, n, k, nq, metric):
    dev = devs(dim, n)
    Q = queries(dim, n, nq)
    dev.set_metric(metric)
    try:
        got, want, fallbacks = batched_and_scan(dev, Q, k, n)
        assert fallbacks == 0  # a bound so loose that random data overflows is a failure too
        assert_same_bits(got, want, (dim, n, k, nq, metric))
        if n == SHAPES[0][0] and dim in (100, 768):  # ... and the scan it equals is the metric's, in float64
            stored = dev.stored_rows(n).cpu().numpy()
            norms = dev.export_rows(0, n)[1].cpu().numpy()
            ref, qn = reference(stored, norms, Q.numpy())
            if metric == "cosine":  # the reference's tolerances are in units of ‖q‖·‖x‖: 1 for a cosine
                qn, norms = np.ones_like(qn), np.ones_like(norms)
            check_against_reference(metric, k, got[0].cpu().numpy(), got[1].cpu().numpy(), ref, qn, norms)
    finally:
        dev.set_metric("cosine")


# ------------------------------------------------------------------ 2. the row-narrowing term
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [512, 768])
def test_row_narrowing_is_in_the_bound(idxmod, cuda, dim, metric):
    """The query is ±1/16 on 256 columns (times 4): qn is f16-exact, so the query-only eps of
    prepare_queries_kernel is its constant 6.5e-5.  k rows among the first 4096 have cosine c0 = 16·b0.
    The planted row has sign(q)·b there, b an f32 just below an f16 rounding midpoint and 2⁻¹⁹ relative
    above b0: its exact cosine is some 28 ulps above c0, and each of the 256 elements loses 2⁻¹⁶ in
    f16, the narrowed dot 2.4e-4.  Every norm is 1, so the three metrics rank alike."""
    import torch

    n, k, planted = FIRST_STAGE + 512, 10, FIRST_STAGE + 300
    rng = np.random.Generator(np.random.PCG64(5))
    sign = np.where(rng.random(256) < 0.5, -1.0, 1.0)
    q = np.zeros(dim, np.float32)
    q[:256] = 4.0 * sign / 16.0
    b = np.nextafter(np.float32(1843.5 * 2.0 ** -15), np.float32(0))  # just below the midpoint of 1843, 1844 (x 2⁻¹⁵)
    b0 = np.float32(float(b) * (1.0 - 2.0 ** -19))
    assert np.float16(b) == np.float16(1843 * 2.0 ** -15) and b0 < b

    def row(beta):  # unit to f32 rounding: sign·beta where q lives, the rest of the norm on the other columns
        x = np.zeros(dim)
        x[:256] = sign * float(beta)
        tail = rng.standard_normal(dim - 256)
        x[256:] = tail / np.linalg.norm(tail) * np.sqrt(1.0 - 256 * float(beta) ** 2)
        return x.astype(np.float32)

    X = rng.standard_normal((n, dim)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    holders = np.arange(100, 100 + 37 * k, 37)
    X[holders] = row(b0)
    X[planted] = row(b)
    qn = q.astype(np.float64) / 4.0
    c0, narrowed = float(qn @ X[holders[0]].astype(np.float64)), float(qn @ X[planted].astype(np.float16).astype(np.float64))
    assert float(qn @ X[planted].astype(np.float64)) > c0  # the planted row belongs to the top k ...
    assert narrowed < c0 - 6.5e-5  # ... and a bound without the row term (thr = c0 - 6.5e-5) would drop it
    dev = idxmod.DeviceIndex(dim, dtype="float32", capacity=n, device=cuda, metric=metric)
    dev.import_rows(0, torch.from_numpy(X).view(torch.uint8), torch.ones(n))  # the stored bits themselves, norms 1
    dev.set_filter("f32")
    got, want, fallbacks = batched_and_scan(dev, torch.from_numpy(q[None]), k, n)
    assert fallbacks == 0
    assert planted in want[1][0].tolist()
    assert planted in got[1][0].tolist()
    assert_same_bits(got, want, (dim, metric))
    dev.close()


# ------------------------------------------------------------------ 3. the bound itself
@pytest.mark.parametrize("dim", [512, 768])
def test_filter_scores_stay_inside_eps(idxmod, cuda, dim):
    """Rows 0-7 have their last 3/4 scaled to ~1e-6 before normalising (f16 subnormals); row 8's columns
    from 64 on are ±5.5e-5, just below f16's normal range, and query 0 is that sign pattern: were those
    flushed to zero (by the conversion or the MFMA) its s' would be short by 5.5e-5·sqrt(dim - 64) > 1e-3."""
    import torch

    n, nq = 4096, 16
    rng = np.random.Generator(np.random.PCG64(7 + dim))
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X[:8, dim // 4:] *= np.float32(1e-6)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    sign = np.where(rng.random(dim - 64) < 0.5, -1.0, 1.0).astype(np.float32)
    X[8, 64:] = np.float32(5.5e-5) * sign
    X[8, :64] *= np.sqrt(1.0 - float(np.sum(X[8, 64:].astype(np.float64) ** 2))) / np.linalg.norm(X[8, :64])
    Q = rng.standard_normal((nq, dim)).astype(np.float32) * np.geomspace(0.5, 20.0, nq).astype(np.float32)[:, None]
    Q[0] = 0.0
    Q[0, 64:] = sign
    dev = f32_index(idxmod, cuda, X)
    sp, eps = dev.filter_scores(torch.from_numpy(Q), 0, n)
    sp, eps = sp.cpu().numpy().astype(np.float64), eps.cpu().numpy().astype(np.float64)
    stored = dev.stored_rows(n).cpu().numpy().astype(np.float64)
    assert np.all(np.abs(stored[8, 64:]) < 2.0 ** -14) and np.all(np.abs(stored[8, 64:]) > 2.0 ** -15)
    q64 = Q.astype(np.float64)
    c64 = (q64 / np.linalg.norm(q64, axis=1, keepdims=True)) @ stored.T
    err = np.abs(sp - c64)
    print("dim", dim, "max |s' - c64| / eps per query:", np.round((err / eps[:, None]).max(axis=1), 3), "eps:", eps)
    assert np.all(np.isfinite(eps)) and np.all(eps > 0)
    assert np.all(err <= eps[:, None]), float((err / eps[:, None]).max())
    dev.close()


# ------------------------------------------------------------------ 4. masked
@pytest.mark.parametrize("dim,metric", [(768, "cosine"), (512, "dotproduct"), (128, "euclidean")])
def test_mfma_masked(devs, cuda, dim, metric):
    """A 5 % random mask, and a mask with one 128-row tile eligible (every other tile skips its epilogue)."""
    import torch

    n, k, nq = SHAPES[0]
    dev = devs(dim, n)
    Q = queries(dim, n, nq)
    one_tile = np.zeros(n, bool)
    one_tile[8192:8320] = True
    dev.set_metric(metric)
    try:
        for eligible in (np.random.Generator(np.random.PCG64(23)).random(n) < 0.05, one_tile):
            words = np.packbits(np.pad(eligible, (0, -n % 32)), bitorder="little").view(np.int32)
            mask = torch.from_numpy(words.copy()).to(cuda)
            got, want, _ = batched_and_scan(dev, Q, k, n, mask=mask, mode="mfma_masked")
            assert_same_bits(got, want, (dim, metric, int(eligible.sum())))
            rows = got[1].cpu().numpy()
            assert rows.min() >= 0 and eligible[rows].all()
    finally:
        dev.set_metric("cosine")


# ------------------------------------------------------------------ 5. fallback
@pytest.mark.parametrize("metric", ["cosine", "dotproduct"])
def test_duplicate_rows_take_the_fallback(idxmod, cuda, metric):
    """4200 copies of one row past the first stage: its query's list overflows the 4096 slots and the
    flagged query runs the f32 (metric) fallback scan."""
    import torch

    dim, (n, k, nq) = 128, SHAPES[0]
    X = data(dim, n)[0].copy()
    X[5000:9200] = X[17]
    dev = f32_index(idxmod, cuda, X, metric)
    Q = queries(dim, n, nq)
    Q[0] = torch.from_numpy(2.0 * X[17])
    got, want, fallbacks = batched_and_scan(dev, Q, k, n)
    assert fallbacks >= 1
    assert_same_bits(got, want, metric)
    dev.close()


# ------------------------------------------------------------------ 6. the public interface
@pytest.mark.parametrize("metric", METRICS)
def test_index_with_the_f32_filter(idxmod, cuda, metric, tmp_path):
    import torch

    dim, (n, k, nq) = 128, SHAPES[0]
    Q = queries(dim, n, nq)
    idx = idxmod.Index("f", dimension=dim, metric=metric, dtype="float32", capacity=n, device=cuda, shards=2, filter="f32")
    assert idx.shard_set.filter == "f32" and idx.shard_set.metric == metric
    idx.upsert_tensor([f"v{i}" for i in range(n)], torch.from_numpy(data(dim, n)[0]).to(cuda))
    want = idx.query_batch(Q, top_k=k, mode="scan")
    assert idx.query_batch(Q, top_k=k, mode="mfma") == want
    idx.save(str(tmp_path))
    back = idxmod.Index.load(str(tmp_path), device=cuda)
    assert back.shard_set.filter == "f32" and back.metric == metric
    assert back.query_batch(Q, top_k=k, mode="mfma") == want
    back.close()
    idx.shard_set.set_filter("native")  # a float32 index has no batched search of its own rows without it
    with pytest.raises(ValueError):
        idx.query_batch(Q, top_k=k, mode="mfma")
    idx.close()
