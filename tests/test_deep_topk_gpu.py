"""GPU tests of the deep top-k (``rc_*_search_deep``: exact results past 256 per query).

Two references, neither of which is the code under test:

* the CHAIN: what a caller had to do before — ``search(k=256, mode="scan", mask=M)`` repeated,
  the returned rows cleared from ``M`` after every call, until ``k`` results or none remain.
  The deep call must equal it bit for bit on scores and exactly on rows, for every ``k``.
* ``oracle.cosine_topk`` on the fetched stored rows under ``topk_equal_modulo_ties`` at 1e-5
  (``test_index_gpu``'s tolerance: both sides score the same stored values; what differs is the
  f32 accumulation).
"""
import numpy as np
import pytest

from conftest import import_pkg
from oracle.cosine_topk import cosine_topk, topk_equal_modulo_ties

pytestmark = pytest.mark.gpu

KS = [257, 511, 512, 513, 1000, 10000]
FORMS = [("float32", "cosine"), ("float16", "cosine"), ("bfloat16", "cosine"), ("f8", "cosine"),
         ("float16", "dotproduct"), ("float16", "euclidean")]


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


@pytest.fixture(scope="module")
def L(cuda):
    return import_pkg("_lib")


def pack(flags):
    return import_pkg("metafilter").pack_bits(np.asarray(flags, dtype=bool))


def dev_mask(words, device):
    import torch

    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32).copy()).to(device)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


_DATA = {}


def data(n, dim, nq, seed):
    """Rows (with distinct norms, so the metrics differ) and queries, once per shape, left unchanged."""
    key = (n, dim, nq, seed)
    if key not in _DATA:
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((n, dim)).astype(np.float32) * rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
        _DATA[key] = (X, rng.standard_normal((nq, dim)).astype(np.float32))
    return _DATA[key]


def make_index(idxmod, cuda, X, dtype, metric="cosine"):
    import torch

    dev = idxmod.DeviceIndex(X.shape[1], dtype=dtype, capacity=X.shape[0] + 3, device=cuda)
    if metric != "cosine":
        dev.set_metric(metric)
    dev.upsert_rows(torch.from_numpy(X), torch.arange(X.shape[0], dtype=torch.int64))
    return dev


def chain(search256, n, k, flags=None):
    """The chain reference for one query: (scores f32 [k], rows i64 [k]), (-inf, -1)-padded.
    ``search256(mask_words)`` is one top-256 masked scan over n rows -> (scores, rows) numpy."""
    elig = np.ones(n, bool) if flags is None else np.asarray(flags, bool).copy()
    out_s, out_r = [], []
    while len(out_r) < k and elig.any():
        s, r = search256(pack(elig))
        live = r >= 0
        assert live.any() and elig[r[live]].all()
        out_s.extend(s[live].tolist())
        out_r.extend(r[live].tolist())
        elig[r[live]] = False
    S = np.full(k, -np.inf, np.float32)
    R = np.full(k, -1, np.int64)
    m = min(k, len(out_r))
    S[:m] = np.asarray(out_s[:m], np.float32)
    R[:m] = out_r[:m]
    return S, R


def dev_chain(dev, q, n, k, flags=None):
    import torch

    def one(words):
        s, r = dev.search(q, 256, n, mode="scan", mask=dev_mask(words, dev.device))
        torch.cuda.synchronize()
        return s.cpu().numpy()[0], r.cpu().numpy()[0]

    return chain(one, n, k, flags)


def deep(dev, q, k, n, mask=None):
    import torch

    s, r = dev.search_deep(q, k, n, mask=mask)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy()


def assert_same(got, want, what):
    gs, gr = got
    ws, wr = want
    assert np.array_equal(gr, wr), (what, np.flatnonzero(gr != wr)[:5], gr[:3], wr[:3])
    assert np.array_equal(bits(gs), bits(ws)), (what, np.flatnonzero(bits(gs) != bits(ws))[:5])


# ------------------------------------------------ sizes, depths, dtypes, metrics --
# n: tiny, around one top-256 list, several rounds, several selection blocks (5077 = 3 blocks with a
# ragged tail), and the one-block / two-block boundary of the selection kernel +- 1
@pytest.mark.parametrize("dtype,metric", FORMS)
@pytest.mark.parametrize("dim", [64, 300])
@pytest.mark.parametrize("n", [1, 255, 257, 300, 1000, 5077, 2047, 2048, 2049])
def test_deep_equals_the_chain_of_masked_scans(idxmod, L, cuda, dtype, metric, dim, n):
    import torch

    assert L.RC_DEEP_SELECT_ROWS == 2048
    X, Q = data(n, dim, 1, 100 + n)
    dev = make_index(idxmod, cuda, X, dtype, metric)
    q = torch.from_numpy(Q[:1])
    ws, wr = dev_chain(dev, q, n, min(max(KS), n + 300))  # every k's expectation is a prefix of the longest chain
    assert sorted(wr[wr >= 0].tolist()) == list(range(n))  # the chain ran until no row was left
    for k in KS:
        es = np.full(k, -np.inf, np.float32)
        er = np.full(k, -1, np.int64)
        m = min(k, len(wr))
        es[:m], er[:m] = ws[:m], wr[:m]
        gs, gr = deep(dev, q, k, n)
        assert_same((gs[0], gr[0]), (es, er), (dtype, metric, dim, n, k))
        if k > n:  # trailing slots
            assert np.all(gr[0, n:] == -1) and np.all(np.isneginf(gs[0, n:]))
    dev.close()


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16", "f8"])
def test_deep_rows_agree_with_the_float64_oracle_on_the_stored_rows(idxmod, cuda, dtype):
    import torch

    n, dim, k = 5077, 300, 1000
    X, Q = data(n, dim, 2, 7)
    dev = make_index(idxmod, cuda, X, dtype)
    gs, gr = deep(dev, torch.from_numpy(Q), k, n)
    stored = dev.stored_rows(n).cpu().numpy()
    ref_r, ref_s = cosine_topk(stored, Q, k, rows_normalized=True)
    for qi in range(2):
        assert topk_equal_modulo_ties(gr[qi], gs[qi], ref_r[qi], ref_s[qi], 1e-5), qi
        qn = Q[qi].astype(np.float64) / np.linalg.norm(Q[qi].astype(np.float64))
        assert np.allclose(gs[qi], stored[gr[qi]].astype(np.float64) @ qn, atol=1e-5, rtol=0)
        assert np.all(np.diff(gs[qi]) <= 0)
    dev.close()


# ----------------------------------------------------- ties across the rounds --
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_ties_across_round_boundaries_come_out_row_ascending(idxmod, cuda, dtype):
    import torch

    n, dim = 1500, 64
    X, _ = data(n, dim, 1, 31)
    X = X.copy()
    tied = np.sort(np.random.default_rng(5).choice(n, 700, replace=False))
    X[tied] = X[tied[0]]  # 700 identical rows scattered among the others
    dev = make_index(idxmod, cuda, X, dtype)
    q = torch.from_numpy(X[tied[0]][None].copy())  # they score highest: both boundaries (256, 512) fall inside the tie
    for k in (513, 700, 1000, 1500):
        gs, gr = deep(dev, q, k, n)
        assert gr[0, :700].tolist() == tied[:k].tolist(), k  # ascending, none twice, none missing
        assert len(set(bits(gs[0, :700]).tolist())) == 1
        assert len(set(gr[0].tolist())) == k
        assert_same((gs[0], gr[0]), dev_chain(dev, q, n, k), k)
    dev.close()


# --------------------------------------------------- prefix and the score pass --
@pytest.mark.parametrize("dtype,metric", FORMS)
def test_prefix_is_the_scan_and_scores_are_the_score_pass(idxmod, cuda, dtype, metric):
    import torch

    n, dim = 3001, 300
    X, Q = data(n, dim, 3, 3)
    dev = make_index(idxmod, cuda, X, dtype, metric)
    q = torch.from_numpy(Q)
    s256, r256 = dev.search(q, 256, n, mode="scan")
    gs, gr = deep(dev, q, 777, n)
    assert np.array_equal(gr[:, :256], r256.cpu().numpy()) and np.array_equal(bits(gs[:, :256]), bits(s256.cpu().numpy()))
    for qi in range(3):
        sc = dev.scores(q[qi], n).cpu().numpy()
        assert sc.shape == (n,)
        assert np.array_equal(bits(sc[gr[qi]]), bits(gs[qi])), qi
        # and the whole order is the score pass's: score descending, then row ascending
        order = np.lexsort((np.arange(n), -sc.astype(np.float64)))[:777]
        assert np.array_equal(order, gr[qi]), qi
    dev.close()


# ------------------------------------------------------------------------ masks --
@pytest.mark.parametrize("dtype,metric", [("float32", "cosine"), ("f8", "cosine"), ("float16", "euclidean")])
def test_masks_short_empty_and_whole_words_cleared(idxmod, cuda, dtype, metric):
    import torch

    n, dim = 2500, 64
    X, Q = data(n, dim, 1, 9)
    dev = make_index(idxmod, cuda, X, dtype, metric)
    q = torch.from_numpy(Q[:1])
    rng = np.random.default_rng(2)
    few = np.zeros(n, bool)
    few[rng.choice(n, 300, replace=False)] = True  # fewer eligible rows than k
    words = rng.random(n) < 0.7
    for w in range(0, n, 64):  # every other 32-row word emptied
        words[w:w + 32] = False
    cases = {"few": (few, 513), "none": (np.zeros(n, bool), 300), "words": (words, 1000), "one": (np.arange(n) == 2499, 257)}
    for name, (flags, k) in cases.items():
        garbage = pack(flags).copy()
        if n % 32:
            garbage[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(n % 32)  # bits at or past n are not trusted
        gs, gr = deep(dev, q, k, n, mask=dev_mask(garbage, dev.device))
        live = int(min(k, flags.sum()))
        assert np.all(gr[0, live:] == -1) and np.all(np.isneginf(gs[0, live:])), name
        assert flags[gr[0, :live]].all(), name
        assert_same((gs[0], gr[0]), dev_chain(dev, q, n, k, flags), name)
    dev.close()


# ----------------------------------------------------------------------- shards --
@pytest.mark.parametrize("dtype,metric", [("float16", "cosine"), ("float32", "dotproduct")])
def test_three_remote_shards_equal_one_shard(idxmod, cuda, dtype, metric):
    import torch

    n, dim = 1000, 64  # 334 + 333 + 333 rows
    X, Q = data(n, dim, 2, 13)
    one = idxmod.ShardSet(dim, dtype=dtype, capacity_per_shard=n + 8, devices=[cuda], metric=metric)
    three = idxmod.ShardSet(dim, dtype=dtype, capacity_per_shard=n // 3 + 8, devices=[cuda] * 3, metric=metric)
    three.force_remote()
    rows = torch.arange(n, dtype=torch.int64)
    one.upsert_rows(torch.from_numpy(X).cuda(), rows)
    three.upsert_rows(torch.from_numpy(X).cuda(), rows)
    q = torch.from_numpy(Q)
    flags = np.random.default_rng(4).random(n) < 0.4
    for k, mask in [(257, None), (600, None), (1000, None), (2000, None), (300, pack(flags)), (700, pack(flags))]:
        s1, r1 = one.search_deep(q, k, n, mask=mask)
        s3, r3 = three.search_deep(q, k, n, mask=mask)
        torch.cuda.synchronize()
        assert_same((s3.cpu().numpy(), r3.cpu().numpy()), (s1.cpu().numpy(), r1.cpu().numpy()), (k, mask is not None))
        live = min(k, n if mask is None else int(flags.sum()))
        assert np.all(r1.cpu().numpy()[:, live:] == -1) and np.all(r1.cpu().numpy()[:, :live] >= 0)
    # the single shard itself is the chain's (its only shard holds global rows = local rows)
    gs, gr = one.search_deep(q[:1], 600, n)
    torch.cuda.synchronize()
    assert_same((gs.cpu().numpy()[0], gr.cpu().numpy()[0]), dev_chain(one.shard(0), q[:1], n, 600), "one")
    one.close()
    three.close()


# ------------------------------------------------------------------- namespaces --
def ids_of(n, prefix="v"):
    return [f"{prefix}{i}" for i in range(n)]


def matches(res):
    return [(m["id"], np.float32(m["score"]).view(np.uint32).item()) for m in res["matches"]]


@pytest.mark.parametrize("shards", [1, 3])
def test_interleaved_namespaces_equal_a_dense_index_of_their_own(idxmod, cuda, shards):
    import torch

    n, dim = 700 * shards, 64  # three pages per shard, the last one partial
    A, _ = data(n, dim, 1, 21)
    B, Q = data(n, dim, 3, 22)
    meta = [{"bucket": i % 3} for i in range(n)]
    ix = idxmod.Index("deep-ns", dimension=dim, dtype="float16", capacity=64, device=cuda, shards=shards, max_top_k=1000)
    dense = idxmod.Index("deep-dense", dimension=dim, dtype="float16", capacity=64, device=cuda, shards=shards, max_top_k=1000)
    step = 100 * shards
    for i in range(0, n, step):  # alternately: the two namespaces' pages interleave in the pool
        for name, V in (("a", A), ("b", B)):
            ix.upsert_tensor(ids_of(n)[i:i + step], torch.from_numpy(V[i:i + step]).cuda(), meta[i:i + step], namespace=name)
        dense.upsert_tensor(ids_of(n)[i:i + step], torch.from_numpy(B[i:i + step]).cuda(), meta[i:i + step])
    pg = ix._ns["b"].pages
    assert len(pg) >= 3 and list(pg) != list(range(pg[0], pg[0] + len(pg)))  # interleaved with "a"'s
    cases = [(None, 600, n), (None, 1000, n), ({"bucket": {"$in": [0, 2]}}, 400, sum(m["bucket"] != 1 for m in meta)),
             ({"bucket": 1}, 1000, sum(m["bucket"] == 1 for m in meta))]
    for flt, k, elig in cases:
        got = ix.query_batch(Q, top_k=k, filter=flt, namespace="b")
        want = dense.query_batch(Q, top_k=k, filter=flt)
        assert [matches(g) for g in got] == [matches(w) for w in want], (flt, k)
        assert all(len(g["matches"]) == min(k, elig) for g in got)
        first = ix.query_batch(Q, top_k=256, filter=flt, namespace="b", mode="scan")
        assert [matches(g)[:256] for g in got] == [matches(f) for f in first]
        one = ix.query(vector=Q[1].tolist(), top_k=k, filter=flt, namespace="b")
        assert matches(one) == matches(got[1])
    # the dense index's own deep answer is the chain's (single shard: checked on its device index)
    if shards == 1:
        dev = dense.shard_set.shard(0)
        gs, gr = dense.shard_set.search_deep(torch.from_numpy(Q[:1]), 600, n)
        torch.cuda.synchronize()
        assert_same((gs.cpu().numpy()[0], gr.cpu().numpy()[0]), dev_chain(dev, torch.from_numpy(Q[:1]), n, 600), "dense")
    ix.close()
    dense.close()


def test_paged_device_index_equals_the_dense_one_and_its_score_pass(idxmod, cuda):
    """rc_index_search_pages_deep / rc_index_scores_pages on a shuffled page list."""
    import torch

    n, dim = 700, 300
    X, Q = data(n, dim, 2, 41)
    dense = make_index(idxmod, cuda, X, "bfloat16")
    pool = idxmod.DeviceIndex(dim, dtype="bfloat16", capacity=256 * 8, device=cuda)
    page_list = [5, 1, 6]
    rows = np.concatenate([np.arange(256) + 256 * p for p in page_list])[:n]
    pool.upsert_rows(torch.from_numpy(X), torch.from_numpy(rows))
    pool.set_pages(3, page_list)
    q = torch.from_numpy(Q)
    flags = np.random.default_rng(8).random(n) < 0.5
    for k, f in [(300, None), (700, None), (1000, None), (300, flags)]:
        m = None if f is None else dev_mask(pack(f), cuda)
        s, r = pool.search_pages_deep(q, k, 3, n, mask=m)
        torch.cuda.synchronize()
        assert_same((s.cpu().numpy(), r.cpu().numpy()), deep(dense, q, k, n, mask=m), (k, f is not None))
    sp = pool.scores(q[0], n, slot=3).cpu().numpy()
    assert np.array_equal(bits(sp), bits(dense.scores(q[0], n).cpu().numpy()))
    dense.close()
    pool.close()


# ------------------------------------------------------- several queries, chunks --
def test_three_queries_in_one_batch_equal_three_single_calls(idxmod, cuda):
    n, dim = 1200, 64
    X, Q = data(n, dim, 3, 51)
    ix = idxmod.Index("deep-batch", dimension=dim, dtype="float32", capacity=n, device=cuda, max_top_k=1000)
    import torch

    ix.upsert_tensor(ids_of(n), torch.from_numpy(X).cuda())
    got = ix.query_batch(Q, top_k=900)
    for qi in range(3):
        assert matches(got[qi]) == matches(ix.query(vector=Q[qi].tolist(), top_k=900)), qi
        assert matches(got[qi]) == matches(ix.query_batch(Q[qi:qi + 1], top_k=900)[0]), qi
    ix.close()


@pytest.mark.parametrize("shards", [1, 3])
def test_results_do_not_depend_on_the_query_chunks(idxmod, L, cuda, shards):
    """70 queries are two chunks (64 in flight at most): each query's answer is its single call's."""
    import torch

    n, dim, k = 900, 64, 600
    X, Q = data(n, dim, 70, 55)
    ss = idxmod.ShardSet(dim, dtype="float16", capacity_per_shard=n // shards + 8, devices=[cuda] * shards)
    ss.upsert_rows(torch.from_numpy(X).cuda(), torch.arange(n, dtype=torch.int64))
    q = torch.from_numpy(Q)
    flags = np.random.default_rng(6).random(n) < 0.8
    for mask in (None, pack(flags)):
        s, r = ss.search_deep(q, k, n, mask=mask)
        torch.cuda.synchronize()
        s, r = s.cpu().numpy(), r.cpu().numpy()
        for qi in (0, 63, 64, 69):
            s1, r1 = ss.search_deep(q[qi], k, n, mask=mask)
            torch.cuda.synchronize()
            assert_same((s[qi], r[qi]), (s1.cpu().numpy()[0], r1.cpu().numpy()[0]), (qi, mask is not None))
    ss.close()


# --------------------------------------------------------------- public surface --
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_index_query_past_256(idxmod, cuda, metric):
    import torch

    n, dim = 1300, 64
    X, Q = data(n, dim, 1, 61)
    meta = [{"i": i} for i in range(n)]
    ix = idxmod.Index("deep-pub", dimension=dim, metric=metric, capacity=n, device=cuda, max_top_k=1000)
    plain = idxmod.Index("deep-plain", dimension=dim, metric=metric, capacity=n, device=cuda)
    for t in (ix, plain):
        t.upsert_tensor(ids_of(n), torch.from_numpy(X).cuda(), meta)
    q = Q[0].tolist()
    res = ix.query(vector=q, top_k=1000, include_values=True, include_metadata=True)
    ms = res["matches"]
    assert len(ms) == 1000 and len({m["id"] for m in ms}) == 1000
    assert matches(res)[:256] == matches(ix.query(vector=q, top_k=256)) == matches(plain.query(vector=q, top_k=256))
    sc = [m["score"] for m in ms]
    assert sc == sorted(sc, reverse=metric == "cosine")  # Euclidean: squared distances, ascending
    assert min(sc) >= 0.0 or metric == "cosine"
    for m in ms[::97]:
        i = int(m["id"][1:])
        assert m["metadata"] == {"i": i}
        np.testing.assert_allclose(m["values"], X[i], rtol=1e-5, atol=1e-5)
    byid = ix.query(id="v5", top_k=300)
    assert byid["matches"][0]["id"] == "v5" and len(byid["matches"]) == 300
    assert [matches(r) for r in ix.query_batch(Q, top_k=400, mode="mfma")] == [matches(ix.query(vector=q, top_k=400))]
    with pytest.raises(ValueError):
        ix.query_batch(Q, top_k=400, mode="nonsense")
    with pytest.raises(ValueError, match="1000"):
        ix.query(vector=q, top_k=1001)
    with pytest.raises(ValueError, match="1000"):
        ix.query_batch(Q, top_k=1001)
    with pytest.raises(ValueError, match="256"):
        plain.query(vector=q, top_k=257)
    with pytest.raises(ValueError, match="256"):
        plain.query_batch(Q, top_k=257)
    ix.close()
    plain.close()


def test_library_calls_refuse_what_they_refused_and_deep_bounds(idxmod, L, cuda):
    import torch

    X, Q = data(300, 64, 1, 71)
    dev = make_index(idxmod, cuda, X, "float32")
    q = torch.from_numpy(Q)
    with pytest.raises(ValueError):
        dev.search(q, 257, 300)
    with pytest.raises(ValueError):
        dev.search_deep(q, 10001, 300)
    with pytest.raises(ValueError):
        dev.search_deep(q, 0, 300)
    with pytest.raises(ValueError):
        dev.search_deep(q, 300, 10 ** 6)  # n_rows beyond the capacity
    s, r = dev.search_deep(q, 10000, 0)  # no rows: every slot empty
    torch.cuda.synchronize()
    assert np.all(r.cpu().numpy() == -1) and np.all(np.isneginf(s.cpu().numpy()))
    gs, gr = deep(dev, q, 1, 300)  # k below 256 works too, and is the scan's answer
    s1, r1 = dev.search(q, 1, 300, mode="scan")
    assert np.array_equal(gr, r1.cpu().numpy()) and np.array_equal(bits(gs), bits(s1.cpu().numpy()))
    dev.close()


# ------------------------------------------------------------------- workspace --
def test_a_repeated_deep_call_allocates_nothing(idxmod, L, cuda):
    import torch

    n, dim = 3000, 64
    X, Q = data(n, dim, 3, 81)
    lib = L.load()
    dev = make_index(idxmod, cuda, X, "float16")
    three = idxmod.ShardSet(dim, dtype="float16", capacity_per_shard=n // 3 + 8, devices=[cuda] * 3)
    three.force_remote()
    three.upsert_rows(torch.from_numpy(X).cuda(), torch.arange(n, dtype=torch.int64))
    q = torch.from_numpy(Q).cuda()
    mask = pack(np.random.default_rng(1).random(n) < 0.5)
    first = deep(dev, q, 1000, n)
    a3 = three.search_deep(q, 1000, n, mask=mask)
    torch.cuda.synchronize()
    before = lib.rc_alloc_count()
    again = deep(dev, q, 1000, n)
    deep(dev, q[:2], 513, n)  # smaller calls fit the same workspace
    b3 = three.search_deep(q, 1000, n, mask=mask)
    torch.cuda.synchronize()
    assert lib.rc_alloc_count() == before
    assert_same(again, first, "repeat")
    assert_same((b3[0].cpu().numpy(), b3[1].cpu().numpy()), (a3[0].cpu().numpy(), a3[1].cpu().numpy()), "repeat sharded")
    dev.close()
    three.close()
