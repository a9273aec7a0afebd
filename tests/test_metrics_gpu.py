"""GPU tests of the index's dotproduct and euclidean metrics (``rc_index_set_metric``): the scan
and the one-launch query form each row's score by the metric's rule before the top-k, so the list
is the metric's own top-k, on every search path and under sharding, masks, persistence and
switching.

Data: ``PCG64(1907)``; rows are ``standard_normal((n, dim))`` scaled per row by ``exp(normal(0, 1))``
(row norms spread over more than a decade, so the cosine, dot and Euclidean top-10 of a query are
almost disjoint: asserted on the reference before any device result is looked at); four queries
scaled by 0.5, 1, 3 and 20.

Reference: float64 on what the device stores — ``stored_rows`` (x̂ as f32) and the exported f32
norms n_r: with qn = ‖q‖ and c = (q / qn) · x̂_r, dot = qn·n_r·c and euclidean = qn² − 2·qn·n_r·c
+ n_r² (the squared distance to the vector ``fetch`` returns).

Tolerances: the project's cosine tolerance of 1e-5 (``test_index_gpu._check``) propagated through
the rule, plus the f32 rounding of the two FMAs relative to the magnitudes they combine:
dot 2e-5·qn·n_r + 1e-6·|ref|, euclidean 2e-5·qn·n_r + 1e-6·(qn + n_r)².  The boundary tolerance
of ``topk_equal_modulo_ties`` is the same expression with n_r at its maximum over the rows (and,
for dot, |ref| at its bound qn·max n_r).
"""
import numpy as np
import pytest

from conftest import import_pkg
from oracle.cosine_topk import topk_equal_modulo_ties

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float16", "bfloat16"]
METRICS = ["dotproduct", "euclidean"]
SHAPES = [(128, 1000), (512, 1000), (768, 3000)]  # nch 1, the VGPR-capped nch 4, nch 6 and several scan blocks
QSCALE = np.array([0.5, 1.0, 3.0, 20.0])


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


_DATA = {}


def data(dim, n):
    """Rows and queries, computed once per shape and left unchanged."""
    if (dim, n) not in _DATA:
        rng = np.random.Generator(np.random.PCG64(1907))
        X = rng.standard_normal((n, dim)) * np.exp(rng.normal(0.0, 1.0, n))[:, None]
        Q = rng.standard_normal((4, dim)) * QSCALE[:, None]
        _DATA[dim, n] = (X.astype(np.float32), Q.astype(np.float32))
    return _DATA[dim, n]


def reference(stored, norms, Q):
    """float64 scores [nq, n] of every row under the three metrics, higher = better (the
    library's convention: Euclidean is the negated squared distance), and qn [nq]."""
    q = Q.astype(np.float64)
    qn = np.linalg.norm(q, axis=1)
    c = (q / qn[:, None]) @ stored.astype(np.float64).T
    nr = norms.astype(np.float64)[None, :]
    return {"cosine": c, "dotproduct": qn[:, None] * nr * c,
            "euclidean": -(qn[:, None] ** 2 - 2.0 * qn[:, None] * nr * c + nr ** 2)}, qn


def tolerance(metric, qn, nr, ref):
    if metric == "dotproduct":
        return 2e-5 * qn * nr + 1e-6 * np.abs(ref)
    return 2e-5 * qn * nr + 1e-6 * (qn + nr) ** 2


def top(scores, k, eligible=None):
    """Rows of the k best scores, score descending then row ascending (all rows if fewer)."""
    rows = np.arange(scores.shape[0]) if eligible is None else np.flatnonzero(eligible)
    order = np.lexsort((rows, -scores[rows]))[:k]
    return rows[order]


_DEVS = {}


@pytest.fixture(scope="module")
def devs(idxmod, cuda):
    """DeviceIndex per (dim, n, dtype) with its stored rows, norms and references: built once."""
    import torch

    def get(dim, n, dtype):
        key = (dim, n, dtype)
        if key not in _DEVS:
            X, Q = data(dim, n)
            dev = idxmod.DeviceIndex(dim, dtype=dtype, capacity=n, device=cuda)
            dev.upsert_rows(torch.from_numpy(X), torch.arange(n))
            stored = dev.stored_rows(n).cpu().numpy()
            _, norms = dev.export_rows(0, n)
            torch.cuda.synchronize()
            norms = norms.cpu().numpy()
            ref, qn = reference(stored, norms, Q)
            _DEVS[key] = (dev, norms, ref, qn)
        return _DEVS[key]

    yield get
    for dev, *_ in _DEVS.values():
        dev.close()
    _DEVS.clear()


def check_against_reference(metric, k, got_s, got_r, ref, qn, norms, eligible=None):
    """got_s / got_r [nq, k] in the library's convention (descending; -inf / -1 past the rows)."""
    n_live = norms.shape[0] if eligible is None else int(eligible.sum())
    kk = min(k, n_live)
    nmax = float(norms.max())
    for q in range(got_s.shape[0]):
        want = top(ref[metric][q], kk, eligible)
        bound = qn[q] * nmax if metric == "dotproduct" else 0.0
        tol_kth = float(tolerance(metric, qn[q], nmax, bound))
        rows = got_r[q, :kk]
        assert np.all(rows >= 0) and len(set(rows.tolist())) == kk, (q, rows)
        if eligible is not None:
            assert np.all(eligible[rows]), (q, rows)
        assert topk_equal_modulo_ties(rows, got_s[q, :kk], want, ref[metric][q][want], tol_kth), (q, rows, want)
        r = ref[metric][q][rows]
        err = np.abs(got_s[q, :kk].astype(np.float64) - r)
        tol = tolerance(metric, qn[q], norms[rows].astype(np.float64), r)
        assert np.all(err <= tol), (q, float((err / tol).max()))
        assert np.all(np.diff(got_s[q, :kk]) <= 0), "scores not descending"
        assert np.all(got_r[q, kk:] == -1) and np.all(np.isneginf(got_s[q, kk:]))


# ------------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("k", [10, 100, 200])  # list sizes 128, 256, 512
@pytest.mark.parametrize("dim,n", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_scan_matches_reference(devs, metric, dtype, dim, n, k):
    import torch

    dev, norms, ref, qn = devs(dim, n, dtype)
    Q = data(dim, n)[1]
    # on the reference alone: the metric's top-10 is not the cosine top-10, for every query, so a
    # build that ignores the metric cannot pass
    for q in range(Q.shape[0]):
        assert set(top(ref[metric][q], 10).tolist()) != set(top(ref["cosine"][q], 10).tolist()), q
    dev.set_metric(metric)
    try:
        s, r = dev.search(torch.from_numpy(Q), k, n, mode="scan")
        check_against_reference(metric, k, s.cpu().numpy(), r.cpu().numpy(), ref, qn, norms)
    finally:
        dev.set_metric("cosine")


# ------------------------------------------------------------------ 2. edge sizes
@pytest.mark.parametrize("n", [1, 31, 33])
@pytest.mark.parametrize("metric", METRICS)
def test_edge_sizes(idxmod, cuda, metric, n):
    import torch

    dim, k = 100, 40  # a padded row width; k > n
    X, Q = data(dim, 64)
    X = X[:n]
    dev = idxmod.DeviceIndex(dim, capacity=64, device=cuda, metric=metric)
    dev.upsert_rows(torch.from_numpy(X), torch.arange(n))
    stored = dev.stored_rows(n).cpu().numpy()
    norms = dev.export_rows(0, n)[1].cpu().numpy()
    ref, qn = reference(stored, norms, Q)
    s, r = dev.search(torch.from_numpy(Q), k, n, mode="scan")
    check_against_reference(metric, k, s.cpu().numpy(), r.cpu().numpy(), ref, qn, norms)  # n live slots, then -inf / -1
    dev.close()
    idx = idxmod.Index("edge", dimension=dim, metric=metric, capacity=64, device=cuda)
    idx.upsert([(f"v{i}", X[i].tolist()) for i in range(n)])
    m = idx.query(vector=Q[2].tolist(), top_k=k)["matches"]
    assert [x["id"] for x in m] == [f"v{i}" for i in r[2, :n].tolist()] and len(m) == n
    idx.close()


# ------------------------------------------------------------------ 3. ties
@pytest.mark.parametrize("metric", METRICS)
def test_ties_order_by_row(idxmod, cuda, metric):
    import torch

    dim, n = 128, 1000
    X = data(dim, n)[0].copy()
    v = (30.0 * np.random.Generator(np.random.PCG64(5)).standard_normal(dim)).astype(np.float32)
    for r in (5, 40, 700):  # two scan blocks; 5 and 40 in different waves of the first
        X[r] = v
    dev = idxmod.DeviceIndex(dim, capacity=n, device=cuda, metric=metric)
    dev.upsert_rows(torch.from_numpy(X), torch.arange(n))
    # q = v: the three copies are the best rows under both metrics (distance 0; dot = ||v||^2,
    # above any other row's ||v||·||x||·cos)
    s, r = dev.search(torch.from_numpy(v[None]), 10, n, mode="scan")
    s, r = s.cpu().numpy()[0], r.cpu().numpy()[0]
    assert r[:3].tolist() == [5, 40, 700]
    assert s[:3].view(np.uint32).tolist() == [int(s[:1].view(np.uint32)[0])] * 3
    assert s[3] < s[2]
    dev.close()


# ------------------------------------------------------------------ 4. one answer on every path
def as_lists(matches):
    return [m["id"] for m in matches], np.array([m["score"] for m in matches], np.float32)


@pytest.mark.parametrize("k", [10, 100])  # both list sizes of the one-launch query
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("metric", METRICS)
def test_every_path_gives_the_same_bits(idxmod, cuda, metric, dtype, k):
    import torch

    dim, n = 768, 3000
    X, Q = data(dim, n)
    Q5 = np.concatenate([Q, Q[:1] * np.float32(7.0)])
    ids = [f"v{i}" for i in range(n)]
    dev = idxmod.DeviceIndex(dim, dtype=dtype, capacity=n, device=cuda, metric=metric)
    dev.upsert_rows(torch.from_numpy(X), torch.arange(n))
    s, r = dev.search(torch.from_numpy(Q5), k, n, mode="scan")
    s, r = s.cpu().numpy(), r.cpu().numpy()
    if metric == "euclidean":  # what Index reports
        assert np.all(s <= 0)
        s = np.maximum(np.float32(0.0), -s)
    dev.close()
    one = idxmod.Index("one", dimension=dim, metric=metric, dtype=dtype, capacity=n, device=cuda)
    many = idxmod.Index("many", dimension=dim, metric=metric, dtype=dtype, capacity=n, device=cuda, shards=3)
    many.shard_set.force_remote()
    xt = torch.from_numpy(X).to(cuda)
    for ix in (one, many):
        ix.upsert_tensor(ids, xt)
        assert ix.shard_set.metric == metric
    batch = {"one": one.query_batch(torch.from_numpy(Q5), top_k=k, mode="scan"),
             "many": many.query_batch(torch.from_numpy(Q5), top_k=k, mode="scan")}
    for q in range(Q5.shape[0]):
        want_ids = [ids[i] for i in r[q].tolist()]
        paths = {"query1": as_lists(one.query(vector=Q5[q].tolist(), top_k=k)["matches"]),  # the one-launch path
                 "sharded": as_lists(many.query(vector=Q5[q].tolist(), top_k=k)["matches"]),
                 "batch": as_lists(batch["one"][q]["matches"]),
                 "sharded batch": as_lists(batch["many"][q]["matches"])}
        for name, (got_ids, got_s) in paths.items():
            assert got_ids == want_ids, (name, q)
            assert got_s.view(np.uint32).tolist() == s[q].view(np.uint32).tolist(), (name, q)
    one.close()
    many.close()


# ------------------------------------------------------------------ 5. masked
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("metric", METRICS)
def test_metadata_filter(idxmod, cuda, metric, dtype):
    dim, n, k = 512, 1000, 10
    X, Q = data(dim, n)
    idx = idxmod.Index("m", dimension=dim, metric=metric, dtype=dtype, capacity=n, device=cuda)
    # "third": every third row; "run": alternate runs of 24 rows (whole 8-row groups stay clear)
    idx.upsert([(f"v{i}", X[i].tolist(), {"third": i % 3, "run": (i // 24) % 2}) for i in range(n)])
    dev = idx.shard_set.shard(0)
    stored = dev.stored_rows(n).cpu().numpy()
    norms = dev.export_rows(0, n)[1].cpu().numpy()
    ref, qn = reference(stored, norms, Q)
    sign = -1.0 if metric == "euclidean" else 1.0
    for flt, eligible in (({"third": 0}, np.arange(n) % 3 == 0), ({"run": 1}, (np.arange(n) // 24) % 2 == 1)):
        for q in range(Q.shape[0]):
            m = idx.query(vector=Q[q].tolist(), top_k=k, filter=flt)["matches"]
            rows = np.array([int(x["id"][1:]) for x in m])
            sc = np.array([x["score"] for x in m], np.float32)
            if metric == "euclidean":
                assert np.all(sc >= 0)
            check_against_reference(metric, k, (sign * sc)[None], rows[None], {metric: ref[metric][q:q + 1]}, qn[q:q + 1],
                                    norms, eligible)
            # an eligible row's score has the bits the unmasked search gives it
            full = {x["id"]: x["score"] for x in idx.query(vector=Q[q].tolist(), top_k=256)["matches"]}
            for x in m:
                assert x["id"] in full and np.float32(full[x["id"]]).view(np.uint32) == np.float32(x["score"]).view(np.uint32)
    idx.close()


# ------------------------------------------------------------------ 6. Euclidean through Index
def test_euclidean_scores_are_squared_distances(idxmod, cuda):
    dim, n = 128, 1000
    X, Q = data(dim, n)
    idx = idxmod.Index("e", dimension=dim, metric="euclidean", capacity=n, device=cuda)
    idx.upsert([(f"v{i}", X[i].tolist()) for i in range(n)])
    for q in range(Q.shape[0]):
        sc = [m["score"] for m in idx.query(vector=Q[q].tolist(), top_k=50)["matches"]]
        assert len(sc) == 50 and min(sc) >= 0.0 and all(a <= b for a, b in zip(sc, sc[1:])), q  # ascending distances
    for vid in ("v0", "v17", "v999"):
        v = idx.fetch([vid])["vectors"][vid]["values"]
        nv = float(np.linalg.norm(np.array(v, np.float64)))
        by_vec = idx.query(vector=v, top_k=5)["matches"]
        assert by_vec[0]["id"] == vid
        assert 0.0 <= by_vec[0]["score"] <= 2e-5 * nv * nv + 1e-6 * (2 * nv) ** 2  # the tolerance at qn = n_r, ref = 0
        assert idx.query(id=vid, top_k=5)["matches"] == by_vec
    # delete works unchanged: the best match leaves, the runner-up keeps its bits and moves up
    before = idx.query(vector=Q[1].tolist(), top_k=3)["matches"]
    idx.delete(ids=[before[0]["id"]])
    after = idx.query(vector=Q[1].tolist(), top_k=2)["matches"]
    assert after == before[1:]
    idx.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals(idxmod, cuda):
    import torch

    X, Q = data(512, 1000)
    with pytest.raises(ValueError):
        idxmod.Index("x", dimension=512, metric="manhattan", device=cuda)
    with pytest.raises(ValueError):
        idxmod.Index("x", dimension=512, metric="dotproduct", filter="i8", device=cuda)
    idx = idxmod.Index("x", dimension=512, metric="dotproduct", dtype="float16", capacity=1000, device=cuda)
    idx.upsert_tensor([f"v{i}" for i in range(1000)], torch.from_numpy(X).to(cuda))
    with pytest.raises(ValueError):
        idx.query_batch(torch.from_numpy(Q), top_k=5, mode="mfma")
    with pytest.raises(ValueError):
        idx.shard_set.shard(0).search(torch.from_numpy(Q), 5, 1000, mode="mfma")
    with pytest.raises(ValueError):
        idx.shard_set.set_filter("i8")
    with pytest.raises(ValueError):
        idx.shard_set.shard(0).set_filter("i8")
    assert idx.shard_set.filter == "native" and idx.shard_set.metric == "dotproduct"
    assert len(idx.query_batch(torch.from_numpy(Q), top_k=5, mode="auto")[0]["matches"]) == 5  # auto scans
    assert idx._masked_mode("auto", 64, 1 << 20, 1 << 20) == "scan"  # where a cosine f16 index would pick MFMA
    idx.close()
    cos = idxmod.Index("c", dimension=512, dtype="float16", capacity=1000, device=cuda, filter="i8")
    with pytest.raises(ValueError):  # the int8 copy exists: no non-cosine metric, on any shard
        cos.shard_set.set_metric("euclidean")
    assert cos.shard_set.metric == "cosine"
    cos.close()


@pytest.mark.parametrize("metric", METRICS)
def test_one_process_per_gpu_index_takes_the_metric(cuda, devs, metric):
    """``sharded.ShardedIndex(metric=)`` hands the metric to its ``DeviceIndex`` (one rank here:
    the merge is not involved, and needs no change — the keys carry the final scores)."""
    import torch

    dim, n, k = 128, 1000, 10
    X, Q = data(dim, n)
    _, norms, ref, qn = devs(dim, n, "float32")
    sh = import_pkg("sharded").ShardedIndex(dim, dtype="float32", capacity_per_rank=n, device=cuda, metric=metric)
    assert sh.local.metric == metric
    sh.upsert_rows(torch.from_numpy(X), torch.arange(n))
    s, r = sh.search(torch.from_numpy(Q), k, mode="scan")
    check_against_reference(metric, k, s.cpu().numpy(), r.cpu().numpy(), ref, qn, norms)
    sh.close()
    with pytest.raises(ValueError):
        import_pkg("sharded").ShardedIndex(dim, capacity_per_rank=n, device=cuda, metric="manhattan")


# ------------------------------------------------------------------ 8. save / load
@pytest.mark.parametrize("metric", METRICS)
def test_save_load_keeps_the_metric(idxmod, cuda, metric, tmp_path):
    dim, n = 128, 1000
    X, Q = data(dim, n)
    idx = idxmod.Index("s", dimension=dim, metric=metric, dtype="float16", capacity=n, device=cuda)
    idx.upsert([(f"v{i}", X[i].tolist(), {"i": i}) for i in range(n)])
    idx.save(str(tmp_path))
    back = idxmod.Index.load(str(tmp_path), device=cuda, shards=2)
    assert back.metric == metric and back.shard_set.metric == metric
    for q in range(Q.shape[0]):
        assert back.query(vector=Q[q].tolist(), top_k=20, include_metadata=True) == \
            idx.query(vector=Q[q].tolist(), top_k=20, include_metadata=True)
    idx.close()
    back.close()


# ------------------------------------------------------------------ 9. switching
def test_set_metric_on_a_populated_index(devs):
    import torch

    dim, n, k = 512, 1000, 10
    dev, norms, ref, qn = devs(dim, n, "float32")
    Q = torch.from_numpy(data(dim, n)[1])
    assert dev.metric == "cosine"
    s0, r0 = dev.search(Q, k, n, mode="scan")
    try:
        for metric in ("dotproduct", "euclidean", "dotproduct"):
            dev.set_metric(metric)
            assert dev.metric == metric
            s, r = dev.search(Q, k, n, mode="scan")
            check_against_reference(metric, k, s.cpu().numpy(), r.cpu().numpy(), ref, qn, norms)
    finally:
        dev.set_metric("cosine")
    s1, r1 = dev.search(Q, k, n, mode="scan")
    assert torch.equal(r0, r1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32))
    for q in range(Q.shape[0]):  # and it is the cosine reference
        assert topk_equal_modulo_ties(r1[q].cpu().numpy(), s1[q].cpu().numpy(), top(ref["cosine"][q], k),
                                      ref["cosine"][q][top(ref["cosine"][q], k)])
