"""GPU tests of the sparse-dense hybrid search (``rc_*_search_hybrid``, the sparse add kernel).

The ORACLE never runs the new kernel.  For a query with dense part ``q`` and sparse part ``sq`` it
takes ``d`` from ``DeviceIndex.scores`` (the deep search's score pass, unchanged code), ``t`` from
``sparsevalues.model_term`` (numpy float32, sequential and unfused), forms ``f32(d + t)`` for the
rows that hold sparse entries when the query holds any (every other row keeps ``d``), and sorts on
the host by (score descending, row ascending) under the mask.  Rows and score BITS must match.
"""
import numpy as np
import pytest

from conftest import import_pkg

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float16", "bfloat16", "f8"]
BIG = 2 ** 32 - 2  # the largest index a record or a query may carry


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


@pytest.fixture(scope="module")
def sv(cuda):
    return import_pkg("sparsevalues")


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


def bits1(x) -> int:
    return int(np.float32(x).view(np.uint32))


def sp_dict(idx, val):
    return {"indices": [int(i) for i in idx], "values": [float(np.float32(v)) for v in val]}


_DATA = {}


def dense(n, dim, nq, seed):
    key = (n, dim, nq, seed)
    if key not in _DATA:
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((n, dim)).astype(np.float32) * rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
        _DATA[key] = (X, rng.standard_normal((nq, dim)).astype(np.float32))
    return _DATA[key]


def vocabulary(size, seed):
    """``size`` distinct indices that include 0 and 2^32 - 2, spread over the whole range."""
    rng = np.random.default_rng(seed)
    rest = rng.permutation(np.unique(rng.integers(1, BIG, 2 * size, dtype=np.int64)))[:size - 2]
    assert rest.shape[0] == size - 2
    return np.concatenate([[0, BIG], rest]).astype(np.int64)


def sparse_rows(n, W, vocab, seed):
    """Row r holds 0 (r % 3 == 0), 1 (r % 3 == 1) or exactly W (r % 3 == 2: no padding) entries."""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(n):
        cnt = (0, 1, W)[r % 3]
        if cnt == 0:
            rows.append(None)
            continue
        idx = rng.choice(vocab[:max(W, 8)] if cnt == W else vocab[:8], cnt, replace=False)
        rows.append(sp_dict(idx, rng.standard_normal(cnt) * 3))
    return rows


def sparse_query(nnz, vocab, seed):
    """A query of nnz entries; the first ones come from the front of the vocabulary (where the rows
    draw theirs), so entries match; nnz = 0 gives None."""
    if nnz == 0:
        return None
    rng = np.random.default_rng(seed)
    return sp_dict(vocab[:nnz], rng.standard_normal(nnz) * 2)


def terms(sv, rows_sp, q_sp):
    """The model's sparse term per row (None where the row keeps d's bits)."""
    if q_sp is None:
        return [None] * len(rows_sp)
    return [None if r is None else sv.model_term(r["indices"], r["values"], q_sp["indices"], q_sp["values"]) for r in rows_sp]


def expected_scores(d, t):
    out = np.asarray(d, np.float32).copy()
    with np.errstate(over="ignore"):
        for r, tr in enumerate(t):
            if tr is not None:
                out[r] = np.float32(out[r] + tr)
    return out


def oracle_topk(sc, k, flags=None):
    n = sc.shape[0]
    order = np.lexsort((np.arange(n), -sc.astype(np.float64)))
    if flags is not None:
        order = order[np.asarray(flags, bool)[order]]
    S = np.full(k, -np.inf, np.float32)
    R = np.full(k, -1, np.int64)
    m = min(k, order.shape[0])
    S[:m], R[:m] = sc[order[:m]], order[:m]
    return S, R


def make_dev(idxmod, cuda, X, dtype, W, rows_sp, extra=3):
    import torch

    n = X.shape[0]
    dev = idxmod.DeviceIndex(X.shape[1], dtype=dtype, capacity=n + extra, device=cuda, metric="dotproduct")
    dev.upsert_rows(torch.from_numpy(X), torch.arange(n, dtype=torch.int64))
    dev.sparse_enable(W)
    assert dev.sparse_width == W
    dev.sparse_write(np.arange(n), rows_sp)
    return dev


def assert_same(got, want, what):
    gs, gr = got
    ws, wr = want
    assert np.array_equal(gr, wr), (what, np.flatnonzero(gr != wr)[:5], gr[:5], wr[:5])
    assert np.array_equal(bits(gs), bits(ws)), (what, np.flatnonzero(bits(gs) != bits(ws))[:5])


# --------------------------------------------------------------- the kernel alone --
_TERMS = {}


def case(sv, n, W, dim):
    """Rows, their sparse entries, four queries (nnz 0, 1, 7, 1024) and the model's terms: once per
    shape, shared by the dtypes."""
    key = (n, W, dim)
    if key not in _TERMS:
        vocab = vocabulary(1024, 1000 + W)
        rows_sp = sparse_rows(n, W, vocab, 17 * n + W)
        qs = [sparse_query(nnz, vocab, 5 + nnz) for nnz in (0, 1, 7, 1024)]
        _TERMS[key] = (rows_sp, qs, [terms(sv, rows_sp, q) for q in qs])
    return _TERMS[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W", [1, 5, 64])
@pytest.mark.parametrize("n,dim", [(1, 64), (63, 64), (64, 64), (65, 64), (255, 64), (257, 64), (1000, 64), (257, 300)])
def test_scores_hybrid_is_fadd_of_the_score_pass_and_the_model_term(idxmod, sv, cuda, dtype, W, n, dim):
    import torch

    X, Q = dense(n, dim, 1, 100 + n)
    rows_sp, qs, ts = case(sv, n, W, dim)
    dev = make_dev(idxmod, cuda, X, dtype, W, rows_sp)
    q = torch.from_numpy(Q[0])
    d = dev.scores(q, n).cpu().numpy()
    for q_sp, t in zip(qs, ts):
        got = dev.scores_hybrid(q, n, q_sp).cpu().numpy()
        want = expected_scores(d, t)
        nnz = 0 if q_sp is None else len(q_sp["indices"])
        assert np.array_equal(bits(got), bits(want)), (nnz, np.flatnonzero(bits(got) != bits(want))[:5])
        keep = [r for r, tr in enumerate(t) if tr is None]  # rows without entries; every row under the empty query
        assert np.array_equal(bits(got[keep]), bits(d[keep]))
        if nnz and n >= 63:  # the case shows something: the term moved some score
            assert (bits(got) != bits(d)).any(), nnz
    assert any(r is not None and 0 in r["indices"] for r in rows_sp) or n < 63
    assert any(r is not None and BIG in r["indices"] for r in rows_sp) or n < 63
    dev.close()


def test_a_rewrite_replaces_every_slot_and_grow_keeps_the_store(idxmod, sv, cuda):
    import torch

    n, dim, W = 300, 64, 5
    X, Q = dense(n, dim, 1, 3)
    rows_sp, qs, ts = case(sv, n, W, dim)
    dev = make_dev(idxmod, cuda, X, "float32", W, rows_sp)
    q = torch.from_numpy(Q[0])
    d = dev.scores(q, n).cpu().numpy()
    before = dev.scores_hybrid(q, n, qs[2]).cpu().numpy()
    dev.grow(4 * n)  # the slot-major store is re-laid for the new capacity
    assert np.array_equal(bits(dev.scores_hybrid(q, n, qs[2]).cpu().numpy()), bits(before))
    # rows 2, 5 (W entries each) get one entry / none: nothing of the old entries may show
    new = list(rows_sp)
    new[2] = sp_dict([0], [2.0])
    new[5] = None
    dev.sparse_write([2, 5], [new[2], new[5]])
    got = dev.scores_hybrid(q, n, qs[2]).cpu().numpy()
    assert np.array_equal(bits(got), bits(expected_scores(d, terms(sv, new, qs[2]))))
    assert bits(got[5]) == bits(d[5])
    dev.close()


# -------------------------------------------------------------------- the search --
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_search_equals_the_oracle_for_every_k_and_mask(idxmod, sv, cuda, dtype):
    import torch

    n, dim, W = 1000, 64, 5
    X, Q = dense(n, dim, 3, 11)
    rows_sp, qs, ts = case(sv, n, W, dim)
    dev = make_dev(idxmod, cuda, X, dtype, W, rows_sp)
    q = torch.from_numpy(Q)
    q_sp = [qs[2], qs[0], qs[3]]  # 7 entries, none, 1024
    want_sc = [expected_scores(dev.scores(q[i], n).cpu().numpy(), t) for i, t in enumerate([ts[2], ts[0], ts[3]])]
    rng = np.random.default_rng(2)
    short = np.zeros(n, bool)
    short[rng.choice(n, 120, replace=False)] = True  # fewer eligible rows than k = 256 / 300
    words = rng.random(n) < 0.7
    for w in range(0, n, 64):  # every other 32-row word cleared
        words[w:w + 32] = False
    for name, flags in [("all", None), ("short", short), ("none", np.zeros(n, bool)), ("words", words)]:
        mask = None
        if flags is not None:
            garbage = pack(flags).copy()
            garbage[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(n % 32)  # bits at or past n are not trusted
            mask = dev_mask(garbage, dev.device)
        for k in (1, 10, 256, 300):
            s, r = dev.search_hybrid(q, k, n, q_sp, mask=mask)
            torch.cuda.synchronize()
            s, r = s.cpu().numpy(), r.cpu().numpy()
            for i in range(3):
                assert_same((s[i], r[i]), oracle_topk(want_sc[i], k, flags), (name, k, i))
    # the first 256 matches of a larger k are the k = 256 answer
    s300, r300 = dev.search_hybrid(q, 300, n, q_sp)
    s256, r256 = dev.search_hybrid(q, 256, n, q_sp)
    assert_same((s300.cpu().numpy()[:, :256], r300.cpu().numpy()[:, :256]), (s256.cpu().numpy(), r256.cpu().numpy()), "prefix")
    # no sparse entries anywhere in the call: the deep search, bit for bit
    for k in (10, 300):
        s, r = dev.search_hybrid(q, k, n, [None] * 3)
        ds, dr = dev.search_deep(q, k, n)
        assert_same((s.cpu().numpy(), r.cpu().numpy()), (ds.cpu().numpy(), dr.cpu().numpy()), ("empty", k))
    dev.close()


def test_the_sparse_term_reorders_the_dense_top_10(idxmod, sv, cuda):
    import torch

    n, dim, W = 1000, 64, 5
    X, Q = dense(n, dim, 1, 23)
    q = torch.from_numpy(Q[:1])
    plain = make_dev(idxmod, cuda, X, "float32", W, [None] * n)
    ds, dr = plain.search_deep(q, 10, n)
    d = plain.scores(q[0], n).cpu().numpy()
    dense_top = dr.cpu().numpy()[0]
    worst = np.argsort(d)[:10]  # the ten rows the dense score likes least get a sparse match worth more than the whole spread
    boost = float(d.max() - d.min()) + 1.0
    rows_sp = [None] * n
    for j, r in enumerate(worst):
        rows_sp[r] = sp_dict([42, 77], [boost + j, 1.0])
    plain.sparse_write(np.arange(n), rows_sp)
    q_sp = sp_dict([42], [1.0])
    s, r = plain.search_hybrid(q, 10, n, [q_sp])
    torch.cuda.synchronize()
    got = r.cpu().numpy()[0]
    assert set(got.tolist()) == set(worst.tolist()) and not set(got.tolist()) & set(dense_top.tolist())
    assert_same((s.cpu().numpy()[0], got), oracle_topk(expected_scores(d, terms(sv, rows_sp, q_sp)), 10), "reorder")
    plain.close()


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_tied_hybrid_scores_come_out_row_ascending_across_256(idxmod, sv, cuda, dtype):
    import torch

    n, dim, W = 1000, 64, 5
    X, _ = dense(n, dim, 1, 31)
    X = X.copy()
    tied = np.sort(np.random.default_rng(5).choice(n, 300, replace=False))
    X[tied] = X[tied[0]]  # 300 identical records scattered among the others: the same dense row ...
    rows_sp = [None] * n
    for r in tied:
        rows_sp[r] = sp_dict([3, 9, BIG], [100.0, -1.0, 2.5])  # ... and the same sparse values
    dev = make_dev(idxmod, cuda, X, dtype, W, rows_sp)
    q = torch.from_numpy(X[tied[0]][None].copy())
    q_sp = sp_dict([3, BIG], [50.0, 1.0])
    sc = expected_scores(dev.scores(q[0], n).cpu().numpy(), terms(sv, rows_sp, q_sp))
    for k in (10, 256, 257, 300):
        s, r = dev.search_hybrid(q, k, n, [q_sp])
        torch.cuda.synchronize()
        s, r = s.cpu().numpy()[0], r.cpu().numpy()[0]
        assert r.tolist() == tied[:k].tolist(), k  # ascending, none twice, none missing
        assert len(set(bits(s).tolist())) == 1
        assert_same((s, r), oracle_topk(sc, k), k)
    dev.close()


def test_the_library_refuses_bad_arguments(idxmod, sv, L, cuda):
    import torch

    n, dim = 100, 64
    X, Q = dense(n, dim, 1, 71)
    q = torch.from_numpy(Q)
    ok = sp_dict([1, 5], [1.0, 2.0])
    off = np.array([0, 2], np.int32)
    val = np.array([1.0, 2.0], np.float32)

    def raw(dev, idx, off=off, val=val, k=5):
        qd = q.cuda()
        s = torch.empty((1, k if 0 < k <= 10000 else 1), device="cuda")
        r = torch.empty((1, k if 0 < k <= 10000 else 1), dtype=torch.int64, device="cuda")
        idx = np.asarray(idx, np.uint32)
        return dev.lib.rc_index_search_hybrid(dev.handle, qd.data_ptr(), 1, n, k, None, off.ctypes.data, idx.ctypes.data,
                                              val.ctypes.data, s.data_ptr(), r.data_ptr(), None)

    dev = idxmod.DeviceIndex(dim, capacity=n, device=cuda, metric="dotproduct")
    dev.upsert_rows(torch.from_numpy(X), torch.arange(n, dtype=torch.int64))
    with pytest.raises(ValueError, match="sparse store"):
        dev.search_hybrid(q, 5, n, [ok])  # not enabled
    with pytest.raises(ValueError, match="sparse store"):
        dev.sparse_write([0], [ok])
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            dev.sparse_enable(bad)
    dev.sparse_enable(2)
    with pytest.raises(ValueError):
        dev.sparse_enable(3)  # another width
    dev.sparse_enable(2)  # the same one again is a no-op
    inv = L.RC_ERR_INVALID
    assert raw(dev, [1, 5]) == 0
    assert raw(dev, [5, 1]) == inv  # unsorted
    assert raw(dev, [5, 5]) == inv  # repeated
    assert raw(dev, [1, 2 ** 32 - 1]) == inv  # the padding value
    assert raw(dev, [1, 5], val=np.array([1.0, np.inf], np.float32)) == inv
    assert raw(dev, [1, 5], k=0) == inv and raw(dev, [1, 5], k=10001) == inv
    big = np.arange(1025, dtype=np.uint32)
    assert raw(dev, big, off=np.array([0, 1025], np.int32), val=np.ones(1025, np.float32)) == inv  # more than 1024 entries
    assert raw(dev, [1, 5], off=np.array([1, 2], np.int32)) == inv
    with pytest.raises(ValueError):
        dev.sparse_write([0], [sp_dict([1, 2, 3], [1.0, 1.0, 1.0])])  # more than the width
    with pytest.raises(ValueError):
        dev.sparse_write([n], [ok])  # row out of capacity
    s, r = dev.search_hybrid(q, 7, 0, [ok])  # no rows: every slot empty
    assert np.all(r.cpu().numpy() == -1) and np.all(np.isneginf(s.cpu().numpy()))
    dev.close()
    cos = idxmod.DeviceIndex(dim, capacity=n, device=cuda)
    cos.sparse_enable(2)
    with pytest.raises(ValueError, match="dotproduct"):
        cos.search_hybrid(q, 5, 0, [ok])
    cos.close()


# ------------------------------------------------------------------------ shards --
def test_three_remote_shards_equal_one_shard(idxmod, sv, cuda):
    import torch

    n, dim, W = 1000, 64, 5  # 334 + 333 + 333 rows
    X, Q = dense(n, dim, 3, 13)
    rows_sp, qs, ts = case(sv, n, W, dim)
    q_sp = [qs[2], qs[0], qs[3]]
    one = idxmod.ShardSet(dim, dtype="float16", capacity_per_shard=n + 8, devices=[cuda], metric="dotproduct")
    three = idxmod.ShardSet(dim, dtype="float16", capacity_per_shard=n // 3 + 8, devices=[cuda] * 3, metric="dotproduct")
    three.force_remote()
    rows = torch.arange(n, dtype=torch.int64)
    for ss in (one, three):
        ss.upsert_rows(torch.from_numpy(X).cuda(), rows)
        ss.sparse_enable(W)
        ss.sparse_write(np.arange(n), rows_sp)
    q = torch.from_numpy(Q)
    flags = np.random.default_rng(4).random(n) < 0.4
    for k, mask in [(10, None), (256, None), (300, None), (1000, None), (10, pack(flags)), (300, pack(flags))]:
        s1, r1 = one.search_hybrid(q, k, n, q_sp, mask=mask)
        s3, r3 = three.search_hybrid(q, k, n, q_sp, mask=mask)
        torch.cuda.synchronize()
        assert_same((s3.cpu().numpy(), r3.cpu().numpy()), (s1.cpu().numpy(), r1.cpu().numpy()), (k, mask is not None))
    # the single shard is the oracle's, and the three shards' diagnostic gives the same scores in global row order
    sc3 = three.scores_hybrid(q[0], n, q_sp[0]).cpu().numpy()
    want = expected_scores(one.shard(0).scores(q[0], n).cpu().numpy(), ts[2])
    assert np.array_equal(bits(sc3), bits(want))
    s1, r1 = one.search_hybrid(q[:1], 300, n, q_sp[:1])
    assert_same((s1.cpu().numpy()[0], r1.cpu().numpy()[0]), oracle_topk(want, 300), "one")
    one.close()
    three.close()


# ------------------------------------------------------------------------- pages --
def ids_of(n, prefix="v"):
    return [f"{prefix}{i}" for i in range(n)]


def matches(res):
    return [(m["id"], np.float32(m["score"]).view(np.uint32).item()) for m in res["matches"]]


@pytest.mark.parametrize("shards", [1, 3])
def test_three_interleaved_namespaces_each_equal_a_dense_index_of_their_own(idxmod, sv, cuda, shards):
    import torch

    n, dim, W = 300 * shards, 64, 5  # two pages per shard, the last one partial
    names = ("a", "b", "c")
    vocab = vocabulary(64, 9)
    V = {nm: dense(n, dim, 3, 40 + i)[0] for i, nm in enumerate(names)}
    S = {nm: sparse_rows(n, W, vocab, 50 + i) for i, nm in enumerate(names)}
    Q = dense(n, dim, 3, 40)[1]
    q_sp = [sparse_query(7, vocab, 1), None, sparse_query(64, vocab, 2)]
    meta = [{"bucket": i % 3} for i in range(n)]
    kw = dict(dimension=dim, metric="dotproduct", dtype="float16", capacity=64, device=cuda, shards=shards, max_top_k=1000,
              sparse_max_nnz=W)
    ix = idxmod.Index("hy-ns", **kw)
    own = {nm: idxmod.Index("hy-" + nm, **kw) for nm in names}
    step = 50 * shards
    for i in range(0, n, step):  # in turn: the namespaces' pages interleave in the pool
        for nm in names:
            args = (ids_of(n)[i:i + step], torch.from_numpy(V[nm][i:i + step]).cuda(), meta[i:i + step])
            ix.upsert_tensor(*args, namespace=nm, sparse_values=S[nm][i:i + step])
            own[nm].upsert_tensor(*args, sparse_values=S[nm][i:i + step])
    pg = ix._ns["b"].pages
    assert len(pg) >= 2 and list(pg) != list(range(pg[0], pg[0] + len(pg)))
    for nm in names:
        for flt, k in [(None, 10), (None, 300), ({"bucket": {"$in": [0, 2]}}, 256), ({"bucket": 1}, 300)]:
            got = ix.query_batch(Q, top_k=k, filter=flt, namespace=nm, sparse_vectors=q_sp)
            want = own[nm].query_batch(Q, top_k=k, filter=flt, sparse_vectors=q_sp)
            assert [matches(g) for g in got] == [matches(w) for w in want], (nm, flt, k)
            assert len(got[0]["matches"]) == min(k, n if flt is None else sum((m["bucket"] == 1) == (flt == {"bucket": 1}) for m in meta))
            one = ix.query(vector=Q[2].tolist(), top_k=k, filter=flt, namespace=nm, sparse_vector=q_sp[2])
            assert matches(one) == matches(got[2])
    # and the dense index of its own is the oracle's (one shard: global rows = local rows)
    if shards == 1:
        dev = own["b"].shard_set.shard(0)
        q0 = torch.from_numpy(Q[0])
        sc = expected_scores(dev.scores(q0, n).cpu().numpy(), terms(sv, S["b"], q_sp[0]))
        es, er = oracle_topk(sc, 300)
        got = own["b"].query(vector=Q[0].tolist(), top_k=300, sparse_vector=q_sp[0])
        assert matches(got) == [(f"v{r}", bits1(s)) for s, r in zip(es, er)]
        # the paged diagnostic against the dense one
        ns = ix._ns["b"]
        paged = ix.pool.shard(0).scores_hybrid(q0, n, q_sp[0], slot=ns.slot).cpu().numpy()
        assert np.array_equal(bits(paged), bits(sc))
    ix.close()
    for t in own.values():
        t.close()


# ------------------------------------------------------------------- index level --
def test_index_round_trip_overwrite_delete_reuse_grow_and_persistence(idxmod, sv, cuda, tmp_path):
    import torch

    n, dim, W = 400, 64, 5
    X, Q = dense(n, dim, 2, 61)
    vocab = vocabulary(64, 3)
    S = sparse_rows(n, W, vocab, 8)
    q_sp = sparse_query(7, vocab, 4)
    ix = idxmod.Index("hy-pub", dimension=dim, metric="dotproduct", capacity=64, device=cuda, shards=2, sparse_max_nnz=W)
    # dict items through upsert (capacity 64: the store grows with the index several times)
    items = [{"id": f"v{i}", "values": X[i].tolist(), "metadata": {"i": i}, **({"sparse_values": S[i]} if S[i] else {})}
             for i in range(n)]
    for i in range(0, n, 100):
        ix.upsert(items[i:i + 100])
    assert ix.capacity >= n

    def oracle(index, ids, sparse_by_id, q, qs, k):
        ss = index.shard_set
        d = np.empty(len(ids), np.float32)
        for s in range(ss.n):
            d[s::ss.n] = ss.shard(s).scores(torch.from_numpy(q), ss.shard_rows(s, len(ids))).cpu().numpy()
        es, er = oracle_topk(expected_scores(d, terms(sv, [sparse_by_id.get(v) for v in ids], qs)), k)
        return [(ids[r], bits1(s)) for s, r in zip(es, er) if r >= 0]

    by_id = {f"v{i}": S[i] for i in range(n) if S[i]}
    ids = ids_of(n)
    for k in (10, 256):
        res = ix.query(vector=Q[0].tolist(), top_k=k, sparse_vector=q_sp, include_values=True, include_metadata=True)
        assert matches(res) == oracle(ix, ids, by_id, Q[0], q_sp, k), k
    for m in res["matches"][:20]:  # include_values carries the record's sparse values
        i = int(m["id"][1:])
        assert ("sparse_values" in m) == (S[i] is not None)
        if S[i]:
            order = np.argsort(S[i]["indices"])
            assert m["sparse_values"]["indices"] == [S[i]["indices"][j] for j in order]
            assert m["sparse_values"]["values"] == [S[i]["values"][j] for j in order]
        assert m["metadata"] == {"i": i}
    got = ix.fetch(["v2", "v3"])["vectors"]
    assert "sparse_values" in got["v2"] and "sparse_values" not in got["v3"]  # rows 2 (W entries) and 3 (none)
    assert sorted(got["v2"]["sparse_values"]["indices"]) == got["v2"]["sparse_values"]["indices"]
    # a query without a sparse part takes the old path: the same as a plain dotproduct index gives
    plain = idxmod.Index("hy-plain", dimension=dim, metric="dotproduct", capacity=n, device=cuda, shards=2)
    plain.upsert_tensor(ids, torch.from_numpy(X).cuda())
    for sp in (None, {"indices": [], "values": []}):
        assert matches(ix.query(vector=Q[0].tolist(), top_k=10, sparse_vector=sp)) == matches(plain.query(vector=Q[0].tolist(), top_k=10))
    plain.close()
    # query by id: the id's stored dense and sparse parts
    byid = ix.query(id="v2", top_k=5)
    stored = ix.fetch(["v2"])["vectors"]["v2"]
    assert matches(byid) == matches(ix.query(vector=stored["values"], top_k=5, sparse_vector=stored["sparse_values"]))
    # an overwrite without sparse values clears them
    ix.upsert([("v2", X[2].tolist())])
    by_id.pop("v2")
    assert "sparse_values" not in ix.fetch(["v2"])["vectors"]["v2"]
    assert matches(ix.query(vector=Q[0].tolist(), top_k=10, sparse_vector=q_sp)) == oracle(ix, ids, by_id, Q[0], q_sp, 10)
    # delete: moved rows are scored with their own sparse values
    gone = [f"v{i}" for i in range(5, 200, 7)]
    ix.delete(ids=gone)
    ids = list(ix._ids)
    assert len(ids) == n - len(gone) and not set(gone) & set(ids)
    for v in gone:
        by_id.pop(v, None)
    assert matches(ix.query(vector=Q[1].tolist(), top_k=256, sparse_vector=q_sp)) == oracle(ix, ids, by_id, Q[1], q_sp, 256)
    # rows reused after the delete show none of the old entries
    ix.upsert([(f"new{i}", X[i].tolist()) for i in range(len(gone))])
    ids = list(ix._ids)
    assert len(ids) == n
    assert matches(ix.query(vector=Q[1].tolist(), top_k=256, sparse_vector=q_sp)) == oracle(ix, ids, by_id, Q[1], q_sp, 256)
    # a named namespace beside it, then save / load: the same matches and score bits
    ix.upsert([{"id": "n1", "values": X[0].tolist(), "sparse_values": S[2]}, {"id": "n2", "values": X[1].tolist()}], namespace="other")
    path = str(tmp_path / "snap")
    ix.save(path)
    import json
    import os

    assert json.load(open(os.path.join(path, "manifest.json")))["sparse_max_nnz"] == W
    back = idxmod.Index.load(path, device=cuda, shards=1)
    assert back.sparse_max_nnz == W
    for t in (Q[0], Q[1]):
        for k in (10, 256):
            assert matches(back.query(vector=t.tolist(), top_k=k, sparse_vector=q_sp)) == matches(ix.query(vector=t.tolist(), top_k=k, sparse_vector=q_sp))
    assert matches(back.query(vector=Q[0].tolist(), top_k=2, sparse_vector=q_sp, namespace="other")) == \
        matches(ix.query(vector=Q[0].tolist(), top_k=2, sparse_vector=q_sp, namespace="other"))
    assert back.fetch(["n1"], namespace="other")["vectors"]["n1"]["sparse_values"] == ix.fetch(["n1"], namespace="other")["vectors"]["n1"]["sparse_values"]
    assert back.fetch(["v9"])["vectors"]["v9"].get("sparse_values") == ix.fetch(["v9"])["vectors"]["v9"].get("sparse_values")
    back.close()
    # refusals
    with pytest.raises(ValueError):
        ix.upsert([{"id": "x", "values": X[0].tolist(), "sparse_values": sp_dict(range(W + 1), [1.0] * (W + 1))}])  # nnz > W
    with pytest.raises(ValueError):
        ix.query(vector=Q[0].tolist(), top_k=5, sparse_vector=sp_dict(range(1025), [1.0] * 1025))  # a query's own limit is 1024
    assert "x" not in ix._rows
    ix.close()
    for metric in ("cosine", "euclidean"):
        with pytest.raises(ValueError, match="dotproduct"):
            idxmod.Index("hy-bad", dimension=dim, metric=metric, device=cuda, sparse_max_nnz=W)
    off = idxmod.Index("hy-off", dimension=dim, metric="dotproduct", capacity=8, device=cuda)
    with pytest.raises(ValueError, match="sparse_max_nnz"):
        off.upsert([{"id": "x", "values": X[0].tolist(), "sparse_values": S[2]}])
    off.upsert([("x", X[0].tolist())])
    with pytest.raises(ValueError, match="sparse_max_nnz"):
        off.query(vector=Q[0].tolist(), top_k=1, sparse_vector=q_sp)
    off.save(str(tmp_path / "off"))
    assert "sparse_max_nnz" not in json.load(open(os.path.join(str(tmp_path / "off"), "manifest.json")))
    assert not [f for f in os.listdir(str(tmp_path / "off")) if "sparse" in f]
    off.close()


def test_a_repeated_hybrid_call_allocates_nothing(idxmod, sv, L, cuda):
    import torch

    n, dim, W = 1000, 64, 5
    X, Q = dense(n, dim, 3, 13)
    rows_sp, qs, ts = case(sv, n, W, dim)
    q_sp = [qs[2], qs[0], qs[3]]
    lib = L.load()
    dev = make_dev(idxmod, cuda, X, "float16", W, rows_sp)
    three = idxmod.ShardSet(dim, dtype="float16", capacity_per_shard=n // 3 + 8, devices=[cuda] * 3, metric="dotproduct")
    three.force_remote()
    three.upsert_rows(torch.from_numpy(X).cuda(), torch.arange(n, dtype=torch.int64))
    three.sparse_enable(W)
    three.sparse_write(np.arange(n), rows_sp)
    q = torch.from_numpy(Q).cuda()
    mask = pack(np.random.default_rng(1).random(n) < 0.5)
    a1 = dev.search_hybrid(q, 300, n, q_sp)
    a3 = three.search_hybrid(q, 300, n, q_sp, mask=mask)
    three.sparse_write(np.arange(10), rows_sp[:10])
    torch.cuda.synchronize()
    before = lib.rc_alloc_count()
    b1 = dev.search_hybrid(q, 300, n, q_sp)
    dev.search_hybrid(q[:2], 10, n, q_sp[:2])  # smaller calls fit the same workspace
    b3 = three.search_hybrid(q, 300, n, q_sp, mask=mask)
    three.sparse_write(np.arange(10), rows_sp[:10])
    torch.cuda.synchronize()
    assert lib.rc_alloc_count() == before
    assert_same((b1[0].cpu().numpy(), b1[1].cpu().numpy()), (a1[0].cpu().numpy(), a1[1].cpu().numpy()), "repeat")
    assert_same((b3[0].cpu().numpy(), b3[1].cpu().numpy()), (a3[0].cpu().numpy(), a3[1].cpu().numpy()), "repeat sharded")
    dev.close()
    three.close()


# ---------------------------------------------------------------- float64 sanity --
@pytest.mark.parametrize("dtype", DTYPES)
def test_scores_agree_with_float64_on_the_stored_values(idxmod, sv, cuda, dtype):
    """Each returned score against ``q . v + sum(v_i * w_i)`` in float64 on the STORED values (``v`` =
    what ``fetch_rows`` returns: the dtype-rounded direction times its f32 norm; the sparse values
    are stored as the float32 they were given).

    Dense part: the deep float64 test (``test_deep_topk_gpu``) allows 1e-5 absolute between a
    score and the float64 dot product of the same stored values, for every dtype, on unit queries
    and unit rows — f32 accumulation over at most a few hundred products bounded by 1 in sum of
    magnitudes.  A dotproduct score scales with ``|q| |v|``, so the rows here have norms in
    [0.5, 1] and the queries are unit vectors: the products are bounded as there and the same 1e-5
    holds.  Sparse part: ``t`` is a sequential float32 sum of nnz products, each rounded once
    (relative 2^-24) and each partial sum rounded once, so ``|t - exact| <= nnz * 2^-24 *
    sum|v w|`` to first order; the final ``fadd(d, t)`` adds at most ``2^-24 (|d| + |t|)``, whose
    ``|t|`` part is below another ``2^-24 sum|v w|`` and whose ``|d|`` part (``|d| <= 1``) is
    inside the dense slack.  Together: ``1e-5 + nnz * 2^-23 * sum|v w|`` with nnz >= 1 the number
    of shared indices."""
    import torch

    n, dim, W = 1000, 300, 64
    rng = np.random.default_rng(77)
    X = rng.standard_normal((n, dim))
    X = (X / np.linalg.norm(X, axis=1, keepdims=True) * rng.uniform(0.5, 1.0, (n, 1))).astype(np.float32)
    Q = rng.standard_normal((2, dim))
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    vocab = vocabulary(128, 5)
    rows_sp = sparse_rows(n, W, vocab, 6)
    q_sp = [sparse_query(64, vocab, 7), sparse_query(7, vocab, 8)]
    dev = make_dev(idxmod, cuda, X, dtype, W, rows_sp)
    s, r = dev.search_hybrid(torch.from_numpy(Q), 300, n, q_sp)
    torch.cuda.synchronize()
    s, r = s.cpu().numpy(), r.cpu().numpy()
    stored = dev.fetch_rows(torch.arange(n)).cpu().numpy().astype(np.float64)
    for qi in range(2):
        w = dict(zip(q_sp[qi]["indices"], np.asarray(q_sp[qi]["values"], np.float32).astype(np.float64)))
        assert np.all(np.diff(s[qi]) <= 0) and len(set(r[qi].tolist())) == 300
        for score, row in zip(s[qi], r[qi]):
            exact = float(stored[row] @ Q[qi].astype(np.float64))
            tol = 1e-5
            if rows_sp[row] is not None:
                prods = [float(np.float32(v)) * w[i] for i, v in zip(rows_sp[row]["indices"], rows_sp[row]["values"]) if i in w]
                exact += sum(prods)
                tol += len(prods) * 2.0 ** -23 * sum(abs(p) for p in prods)
            assert abs(float(score) - exact) <= tol, (qi, row, float(score), exact, tol)
    dev.close()
