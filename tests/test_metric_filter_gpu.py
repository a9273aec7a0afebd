"""GPU tests of the metric filter (``rc_index_set_filter(RC_FILTER_METRIC)``): the batched MFMA
search of an f16 / bf16 index under dotproduct and euclidean.  Its filter GEMM bounds each row's
metric score from above, its candidates are rescored by the scan's own rule, so in every test
``mode="mfma"`` must equal ``mode="scan"`` on the same index BIT FOR BIT, scores and rows.

Data as in ``test_metrics_gpu.py``: rows are ``standard_normal((n, dim))`` scaled per row by
``exp(normal(0, 1))``, queries are scaled 0.5 ... 20 (geometrically over the batch), so the three
metrics' top-k differ.  The search's first stage takes the first 4096 rows unfiltered: every shape
has n > 4096, and whatever a test plants sits past row 4096, where the filter decides.
"""
import numpy as np
import pytest

from conftest import import_pkg
from test_metrics_gpu import check_against_reference, reference

pytestmark = pytest.mark.gpu

METRICS = ["dotproduct", "euclidean"]
DTYPES = ["float16", "bfloat16"]
# 128 and 512: filter_qs_metric_kernel at NKT 2 and 8; 768: filter_gemm_metric_kernel (the embedder's
# width); 100: a padded row (ld 128: the NKT 2 kernel again, over zero columns)
DIMS = [128, 512, 768, 100]
# (n, k, nq): a ragged last tile and one padded query block; three stages, the last shorter than a
# chunk; two query blocks and the largest list
SHAPES = [(20_011, 10, 9), (70_000, 100, 20), (70_000, 256, 300)]
# ... and the remaining instantiation, filter_qs_metric_kernel at NKT 4, on the smallest shape
EXTRA = [(256,) + SHAPES[0]]
NQ_MAX = 300
FIRST_STAGE = 4096


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


_DATA = {}


def data(dim, n):
    """Rows [n, dim] and queries [NQ_MAX, dim]; the latest shape only is kept (215 MB at the largest)."""
    if (dim, n) not in _DATA:
        _DATA.clear()
        rng = np.random.Generator(np.random.PCG64(1907 + dim))
        X = rng.standard_normal((n, dim), dtype=np.float32)
        X *= np.exp(rng.normal(0.0, 1.0, n)).astype(np.float32)[:, None]
        Q = rng.standard_normal((NQ_MAX, dim), dtype=np.float32) * np.geomspace(0.5, 20.0, NQ_MAX).astype(np.float32)[:, None]
        _DATA[dim, n] = (X, Q)
    return _DATA[dim, n]


def queries(dim, n, nq):
    import torch

    Q = data(dim, n)[1]
    pick = np.linspace(0, NQ_MAX - 1, nq).round().astype(int)  # every scale, whatever nq
    return torch.from_numpy(np.ascontiguousarray(Q[pick]))


_DEVS = {}


@pytest.fixture(scope="module")
def devs(idxmod, cuda):
    """DeviceIndex with the "metric" filter per (dim, n, dtype): built once, rows left unchanged."""
    import torch

    def get(dim, n, dtype):
        key = (dim, n, dtype)
        if key not in _DEVS:
            dev = idxmod.DeviceIndex(dim, dtype=dtype, capacity=n, device=cuda)
            dev.upsert_rows(torch.from_numpy(data(dim, n)[0]), torch.arange(n))
            dev.set_filter("metric")
            _DEVS[key] = dev
        return _DEVS[key]

    yield get
    for dev in _DEVS.values():
        dev.close()
    _DEVS.clear()


def assert_same_bits(got, want, what=""):
    import torch

    (s, r), (s2, r2) = got, want
    assert torch.equal(r, r2), (what, "rows")
    assert torch.equal(s.view(torch.int32), s2.view(torch.int32)), (what, "score bits")


def mfma_and_scan(dev, Q, k, n, mask=None):
    """(mfma result, scan result, fallbacks of the mfma search)"""
    dev.timing(True)
    dev.gemm_timing_read()
    got = dev.search(Q, k, n, mode="mfma", mask=mask)
    fallbacks = dev.gemm_timing_read()[3]
    dev.timing(False)
    return got, dev.search(Q, k, n, mode="scan", mask=mask), fallbacks


# ------------------------------------------------------------------ 1. shapes
CASES = [(dim, n, k, nq, dtype, metric) for (dim, n, k, nq) in [(d,) + s for d in DIMS for s in SHAPES] + EXTRA
         for dtype in DTYPES for metric in METRICS]


@pytest.mark.parametrize("dim,n,k,nq,dtype,metric", CASES)
def test_mfma_equals_scan(devs, dim, n, k, nq, dtype, metric):
    dev = devs(dim, n, dtype)
    Q = queries(dim, n, nq)
    dev.set_metric(metric)
    try:
        got, want, _ = mfma_and_scan(dev, Q, k, n)
        assert_same_bits(got, want, (dim, n, k, nq, dtype, metric))
        # ... and the scan it equals is the metric's: float64 on what the device stores, test_metrics_gpu's
        # rule and tolerances, on the smallest shape of two widths
        if n == SHAPES[0][0] and dim in (100, 128) and dtype == "float16":
            stored = dev.stored_rows(n).cpu().numpy()
            norms = dev.export_rows(0, n)[1].cpu().numpy()
            ref, qn = reference(stored, norms, Q.numpy())
            check_against_reference(metric, k, got[0].cpu().numpy(), got[1].cpu().numpy(), ref, qn, norms)
    finally:
        dev.set_metric("cosine")


# ------------------------------------------------------------------ 2. boundary ladder
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_boundary_ladder(idxmod, cuda, metric, dtype):
    """3000 rows share one stored direction (identical bits) and have norms one f32 ulp apart,
    1024·(1 + i·2⁻²³): half of them in the second stage's rows, half in the third's (k = 100: the
    stages end at 4096, 65536 and n).  The queries are that direction at a norm inside the ladder,
    so under dotproduct the top-k are the ladder's largest norms (the third stage must let every
    row above the running k-th best through) and under euclidean the ladder rows' scores differ by
    far less than an ulp of ‖q‖² ≈ 10⁶: ties in their hundreds, straddling the stage boundary,
    which only the ``>=`` of the filter test and the row order of the keys resolve as the scan
    does.  The other rows past the first stage are scaled by 1/4, so that few of them pass and the
    ladder's 1500 candidates per stage stay inside the 4096 slots: no fallback."""
    import torch

    dim, n, k = 128, 70_000, 100
    rng = np.random.Generator(np.random.PCG64(11))
    X = data(dim, n)[0].copy()
    X[FIRST_STAGE:] *= np.float32(0.25)
    d = rng.standard_normal(dim).astype(np.float32)
    d /= np.linalg.norm(d)
    spans = [(5_000, 1_500), (66_000, 1_500)]
    for r0, m in spans:
        X[r0:r0 + m] = d
    ladder = (np.float32(1024.0) * (np.float32(1.0) + np.arange(3000, dtype=np.float32) * np.float32(2.0 ** -23))).astype(np.float32)
    assert np.all(np.diff(ladder.view(np.int32)) == 1)  # one ulp apart, exactly
    dev = idxmod.DeviceIndex(dim, dtype=dtype, capacity=n, device=cuda, metric=metric)
    dev.upsert_rows(torch.from_numpy(X), torch.arange(n))
    i0 = 0
    for r0, m in spans:  # identical stored bits, exact norms
        bits, _ = dev.export_rows(r0, 1)
        dev.import_rows(r0, bits.repeat(m, 1), torch.from_numpy(ladder[i0:i0 + m]))
        i0 += m
    dev.set_filter("metric")
    Q = torch.from_numpy(np.stack([d * ladder[j] for j in (500, 1499, 1500, 2500)]))
    got, want, fallbacks = mfma_and_scan(dev, Q, k, n)
    assert fallbacks == 0
    assert_same_bits(got, want, (metric, dtype))
    rows = got[1].cpu().numpy()
    in_ladder = ((rows >= 5_000) & (rows < 6_500)) | ((rows >= 66_000) & (rows < 67_500))
    assert in_ladder.all()  # the k-th best falls inside the ladder
    if metric == "dotproduct":  # the largest norms: all in the third stage's half of the ladder
        assert rows.min() >= 66_000
    dev.close()


# ------------------------------------------------------------------ 3. fallback
@pytest.mark.parametrize("metric", METRICS)
def test_duplicate_rows_take_the_metric_fallback(idxmod, cuda, metric):
    """100 000 rows drawn from 3 base vectors with 3 norms: exact ties in their thousands overflow
    the candidate lists, and the flagged queries run the metric fallback scan (masked=False)."""
    import torch

    rng = np.random.default_rng(3)
    dim, n, k = 512, 100_000, 50
    base = rng.standard_normal((3, dim)).astype(np.float32)
    scale = np.array([0.5, 1.0, 3.0], np.float32)
    X = base[rng.integers(0, 3, n)] * scale[rng.integers(0, 3, n)][:, None]
    dev = idxmod.DeviceIndex(dim, dtype="float16", capacity=n, device=cuda, metric=metric)
    dev.upsert_rows(torch.from_numpy(X), torch.arange(n))
    dev.set_filter("metric")
    Q = torch.from_numpy(np.concatenate([base[:2], 2.0 * base[2:], rng.standard_normal((13, dim)).astype(np.float32)]))
    got, want, fallbacks = mfma_and_scan(dev, Q, k, n)
    assert fallbacks >= 1
    assert_same_bits(got, want, metric)
    dev.close()


# ------------------------------------------------------------------ 4. masked
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_masked(devs, cuda, metric, dtype):
    """Eligible shares 0.6 and 0.05.  At 0.05 the threshold after the first stage is the k-th best
    of some 200 eligible rows, about half of the second stage passes, and the queries overflow
    into the MASKED metric fallback scan."""
    import torch

    dim, n, k, nq = 512, 70_000, 100, 20
    dev = devs(dim, n, dtype)
    Q = queries(dim, n, nq)
    rng = np.random.Generator(np.random.PCG64(23))
    dev.set_metric(metric)
    try:
        for share in (0.6, 0.05):
            eligible = rng.random(n) < share
            words = np.packbits(np.pad(eligible, (0, -n % 32)), bitorder="little").view(np.int32)
            mask = torch.from_numpy(words.copy()).to(cuda)
            got, want, fallbacks = mfma_and_scan(dev, Q, k, n, mask=mask)
            assert_same_bits(got, want, (metric, dtype, share))
            rows = got[1].cpu().numpy()
            assert rows.min() >= 0 and eligible[rows].all()
            if share == 0.05:
                assert fallbacks >= 1
    finally:
        dev.set_metric("cosine")


# ------------------------------------------------------------------ 5. shards
@pytest.mark.parametrize("metric", METRICS)
def test_sharded_index(idxmod, cuda, metric):
    import torch

    dim, n, k, nq = 128, 20_011, 10, 9
    X = data(dim, n)[0]
    Q = queries(dim, n, nq)
    ids = [f"v{i}" for i in range(n)]
    xt = torch.from_numpy(X).to(cuda)
    one = idxmod.Index("one", dimension=dim, metric=metric, dtype="float16", capacity=n, device=cuda)
    many = idxmod.Index("many", dimension=dim, metric=metric, dtype="float16", capacity=n, device=cuda, shards=3, filter="metric")
    assert many.shard_set.filter == "metric" and many.shard_set.metric == metric
    for ix in (one, many):
        ix.upsert_tensor(ids, xt)
    want = one.query_batch(Q, top_k=k, mode="scan")
    for remote in (False, True):
        if remote:
            many.shard_set.force_remote()
        got = many.query_batch(Q, top_k=k, mode="mfma")
        for q in range(nq):
            assert [m["id"] for m in got[q]["matches"]] == [m["id"] for m in want[q]["matches"]], (remote, q)
            sg = np.array([m["score"] for m in got[q]["matches"]], np.float32)
            sw = np.array([m["score"] for m in want[q]["matches"]], np.float32)
            assert sg.view(np.uint32).tolist() == sw.view(np.uint32).tolist(), (remote, q)
            if metric == "euclidean":  # squared distances: positive, nearest first
                assert np.all(sg > 0) and np.all(np.diff(sg) >= 0)
    one.close()
    many.close()


# ------------------------------------------------------------------ 6. auto and switching
@pytest.mark.parametrize("metric", METRICS)
def test_auto_takes_the_batched_path(devs, metric):
    dim, n, k, nq = 512, 70_000, 10, 16
    dev = devs(dim, n, "float16")
    Q = queries(dim, n, nq)
    dev.set_metric(metric)
    try:
        dev.timing(True)
        dev.gemm_timing_read()
        got = dev.search(Q, k, n)  # mode="auto"
        _, launches, flops, _ = dev.gemm_timing_read()
        dev.timing(False)
        assert launches >= 1 and flops > 0
        assert_same_bits(got, dev.search(Q, k, n, mode="scan"), metric)
    finally:
        dev.set_metric("cosine")


@pytest.mark.parametrize("dtype", DTYPES)
def test_switching_metrics_on_a_populated_index(devs, dtype):
    dim, n, k, nq = 512, 70_000, 10, 16
    dev = devs(dim, n, dtype)
    Q = queries(dim, n, nq)
    results = {}
    try:
        for step, metric in enumerate(("cosine", "dotproduct", "euclidean", "cosine")):
            dev.set_metric(metric)
            assert dev.metric == metric and dev.filter == "metric"
            got = dev.search(Q, k, n, mode="mfma")
            assert_same_bits(got, dev.search(Q, k, n, mode="scan"), (step, metric))
            results[step] = got
        assert_same_bits(results[0], results[3], "cosine before and after")
        for a, b in ((0, 1), (0, 2), (1, 2)):  # three different top-k lists
            assert not np.array_equal(results[a][1].cpu().numpy(), results[b][1].cpu().numpy())
        dev.set_filter("native")  # under cosine the "metric" filter is the native one: the same bits
        assert_same_bits(results[0], dev.search(Q, k, n, mode="mfma"), "native")
    finally:
        dev.set_metric("cosine")
        dev.set_filter("metric")


# ------------------------------------------------------------------ 7. refusals and persistence
def test_refusals(idxmod, cuda):
    import torch

    dim, n = 128, 5_000
    X = data(dim, 20_011)[0][:n]
    Q = queries(dim, 20_011, 9)
    for dtype in ("float32", "f8"):
        dev = idxmod.DeviceIndex(dim, dtype=dtype, capacity=n, device=cuda)
        with pytest.raises(ValueError):
            dev.set_filter("metric")
        assert dev.filter == "native"
        dev.close()
    with pytest.raises(ValueError):
        idxmod.Index("x", dimension=dim, dtype="float32", filter="metric", device=cuda)
    idx = idxmod.Index("x", dimension=dim, metric="dotproduct", dtype="float16", capacity=n, device=cuda, shards=2, filter="metric")
    idx.upsert_tensor([f"v{i}" for i in range(n)], torch.from_numpy(X).to(cuda))
    with pytest.raises(ValueError):  # the int8 filter is cosine-only
        idx.shard_set.set_filter("i8")
    with pytest.raises(ValueError):
        idx.shard_set.shard(0).set_filter("i8")
    assert idx.shard_set.filter == "metric" and idx.shard_set.shard(1).filter == "metric"  # the refusal changed nothing
    assert len(idx.query_batch(Q, top_k=5, mode="mfma")[0]["matches"]) == 5
    idx.shard_set.set_filter("native")  # the default: a dotproduct index refuses the batched search
    with pytest.raises(ValueError):
        idx.query_batch(Q, top_k=5, mode="mfma")
    idx.close()


@pytest.mark.parametrize("metric", METRICS)
def test_save_load_keeps_the_filter_and_the_metric(idxmod, cuda, metric, tmp_path):
    import torch

    dim, n = 128, 5_000
    X = data(dim, 20_011)[0][:n]
    Q = queries(dim, 20_011, 9)
    idx = idxmod.Index("s", dimension=dim, metric=metric, dtype="bfloat16", capacity=n, device=cuda, filter="metric")
    idx.upsert_tensor([f"v{i}" for i in range(n)], torch.from_numpy(X).to(cuda))
    idx.save(str(tmp_path))
    back = idxmod.Index.load(str(tmp_path), device=cuda)
    assert back.metric == metric and back.shard_set.metric == metric and back.shard_set.filter == "metric"
    assert back.query_batch(Q, top_k=20, mode="mfma") == idx.query_batch(Q, top_k=20, mode="scan")
    idx.close()
    back.close()
