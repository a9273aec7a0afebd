"""The deep top-k's radix selection (``deep_select="radix"``) against the score pass's f32 scores
(``DeviceIndex.scores``, no selection) ordered on the host: score descending, row ascending, the tail
``(-inf, -1)``; a device index returns those values under every metric.  Rows and score bits are equal."""
import functools

import numpy as np
import pytest
import torch

from conftest import import_pkg

pytestmark = pytest.mark.gpu

FORMS = [("float32", "cosine", 64), ("float16", "euclidean", 64), ("f8", "cosine", 64), ("float16", "cosine", 300)]


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def pack(flags):
    return import_pkg("metafilter").pack_bits(np.asarray(flags, dtype=bool))


@functools.lru_cache(None)
def data(n, dim, seed):
    """Rows with distinct norms and three queries, once per shape; callers copy before they change them."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32) * rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    return X, rng.standard_normal((3, dim)).astype(np.float32)


def make_dev(idxmod, cuda, X, dtype="float32", metric="cosine", select="radix"):
    dev = idxmod.DeviceIndex(X.shape[1], dtype=dtype, capacity=X.shape[0] + 3, device=cuda, metric=metric)
    dev.upsert_rows(torch.from_numpy(X), torch.arange(X.shape[0], dtype=torch.int64))
    dev.set_deep_select(select)
    return dev


def reference(sc, k, flags=None):
    sc = np.asarray(sc, np.float32) + np.float32(0)  # the key folds -0 into +0
    order = np.lexsort((np.arange(sc.shape[0]), -sc.astype(np.float64)))
    if flags is not None:
        order = order[np.asarray(flags, bool)[order]]
    S, R = np.full(k, -np.inf, np.float32), np.full(k, -1, np.int64)
    m = min(k, order.shape[0])
    S[:m], R[:m] = sc[order[:m]], order[:m]
    return S, R


def run(call, *args, **kw):
    s, r = call(*args, **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy()


def assert_same(got, want, what=None):
    assert np.array_equal(got[1], want[1]), (what, np.flatnonzero(got[1] != want[1])[:5])
    assert np.array_equal(bits(got[0]), bits(want[0])), (what, np.flatnonzero(bits(got[0]) != bits(want[0]))[:5])


def check(dev, q, k, n, flags=None, what=None):
    mask = None if flags is None else torch.from_numpy(pack(flags).view(np.int32).copy()).to(dev.device)
    gs, gr = run(dev.search_deep, q, k, n, mask=mask)
    for i in range(q.shape[0]):
        assert_same((gs[i], gr[i]), reference(dev.scores(q[i], n).cpu().numpy(), k, flags), (what, k, i))
    return gs, gr


# n: one entry, around one top-256 list, the one-block / two-block boundary of the passes +- 1,
# three blocks with a ragged tail, ten blocks (15 row bits: two row digits)
@pytest.mark.parametrize("k", [257, 1000, 10000])
@pytest.mark.parametrize("n", [1, 255, 257, 2047, 2049, 5077, 20000])
@pytest.mark.parametrize("dtype,metric,dim", FORMS)
def test_sizes_and_depths(idxmod, cuda, dtype, metric, dim, n, k):
    X, Q = data(n, dim, 100 + n)
    dev = make_dev(idxmod, cuda, X, dtype, metric)
    check(dev, torch.from_numpy(Q[:1]), k, n)
    dev.close()


@pytest.mark.parametrize("k", [257, 1000, 1500, 1650, 1900])
def test_the_cut_in_the_lowest_score_digit(idxmod, cuda, k):
    """Exact dot products one f32 ulp apart: a ladder 1024 (1 + i 2^-23) of 1500 rows, 200 all-zero rows
    (score +0: a tie that k = 1650 cuts by row) and 300 rows of the negated ladder, shuffled."""
    n, dim = 2000, 64
    ladder = (np.float32(1024.0) * (np.float32(1.0) + np.arange(1500, dtype=np.float32) * np.float32(2.0 ** -23))).astype(np.float32)
    X = np.zeros((n, dim), np.float32)
    X[:, 0] = np.random.default_rng(3).permutation(np.concatenate([ladder, np.zeros(200, np.float32), -ladder[:300]]))
    dev = make_dev(idxmod, cuda, X, "float32", "dotproduct")
    q = np.zeros((1, dim), np.float32)
    q[0, 0] = 1.0
    gs, _ = check(dev, torch.from_numpy(q), k, n)
    assert np.array_equal(bits(gs[0]), bits(np.sort(X[:, 0] + np.float32(0))[::-1][:k]))
    dev.close()


@pytest.mark.parametrize("n,tied,k", [(3000, 3000, 1000), (1500, 700, 300), (1500, 700, 699)])
def test_the_cut_inside_a_tie_is_made_by_row(idxmod, cuda, n, tied, k):
    X = data(n, 64, 31)[0].copy()
    rows = np.sort(np.random.default_rng(5).choice(n, tied, replace=False))
    X[rows] = X[rows[0]]  # identical rows scattered among the others; they score highest
    dev = make_dev(idxmod, cuda, X, "float16")
    gs, gr = check(dev, torch.from_numpy(X[rows[:1]].copy()), k, n)
    assert gr[0].tolist() == rows[:k].tolist() and len(set(bits(gs[0]).tolist())) == 1  # ascending, none twice
    dev.close()


@pytest.mark.parametrize("case,k", [("none", 300), ("few", 513), ("words", 1000)])
def test_masks(idxmod, cuda, case, k):
    n = 2500
    X, Q = data(n, 64, 9)
    rng = np.random.default_rng(2)
    flags = np.zeros(n, bool)
    if case == "few":
        flags[rng.choice(n, 300, replace=False)] = True  # fewer eligible rows than k
    if case == "words":
        flags = rng.random(n) < 0.7
        for w in range(0, n, 64):  # every other 32-row word cleared
            flags[w:w + 32] = False
    dev = make_dev(idxmod, cuda, X, "float16", "euclidean")
    _, gr = check(dev, torch.from_numpy(Q[:1]), k, n, flags, case)
    assert np.all(gr[0, int(min(k, flags.sum())):] == -1)
    dev.close()


def test_three_queries_in_one_call_equal_three_single_calls(idxmod, cuda):
    """Dot product: the tied rows' own vector (700 ties on top), a random query, the zero vector (all tie)."""
    n, k = 1500, 900
    X = data(n, 64, 31)[0].copy()
    X[::2][:700] = X[0]
    dev = make_dev(idxmod, cuda, X, "float32", "dotproduct")
    q = torch.from_numpy(np.stack([X[0], data(n, 64, 31)[1][0], np.zeros(64, np.float32)]))
    gs, gr = check(dev, q, k, n)
    for i in range(3):
        assert_same((gs[i:i + 1], gr[i:i + 1]), run(dev.search_deep, q[i:i + 1], k, n), i)
    dev.close()


@pytest.mark.parametrize("k,masked", [(300, False), (1000, False), (2000, False), (700, True)])
def test_three_remote_shards_equal_one_shard(idxmod, cuda, k, masked):
    n, dim = 1000, 64  # 334 + 333 + 333 rows: the leader selects over three lists of k ready keys
    X, Q = data(n, dim, 13)
    one = make_dev(idxmod, cuda, X, "float16")
    three = idxmod.ShardSet(dim, dtype="float16", capacity_per_shard=n // 3 + 8, devices=[cuda] * 3)
    three.force_remote()
    three.set_deep_select("radix")
    three.upsert_rows(torch.from_numpy(X).cuda(), torch.arange(n, dtype=torch.int64))
    flags = np.random.default_rng(4).random(n) < 0.4 if masked else None
    q = torch.from_numpy(Q)
    got = run(three.search_deep, q, k, n, mask=None if flags is None else pack(flags))
    for i in range(3):
        assert_same((got[0][i], got[1][i]), reference(one.scores(q[i], n).cpu().numpy(), k, flags), i)
    one.close()
    three.close()


def matches(res):
    return [(m["id"], np.float32(m["score"]).view(np.uint32).item()) for m in res["matches"]]


def test_an_interleaved_namespace_equals_a_dense_index_of_its_own(idxmod, cuda):
    n, dim, step = 700, 64, 100  # three pages, the last one partial
    A, B = data(n, dim, 21)[0], data(n, dim, 22)[0]
    ids = [f"v{i}" for i in range(n)]
    ix = idxmod.Index("radix-ns", dimension=dim, dtype="float16", capacity=64, device=cuda, max_top_k=1000, deep_select="radix")
    dense = idxmod.Index("radix-dense", dimension=dim, dtype="float16", capacity=64, device=cuda, max_top_k=1000)
    for i in range(0, n, step):  # alternately: the two namespaces' pages interleave in the pool
        for name, V in (("a", A), ("b", B)):
            ix.upsert_tensor(ids[i:i + step], torch.from_numpy(V[i:i + step]).cuda(), namespace=name)
        dense.upsert_tensor(ids[i:i + step], torch.from_numpy(B[i:i + step]).cuda())
    Q = data(n, dim, 22)[1]
    for k in (600, 1000):
        assert [matches(g) for g in ix.query_batch(Q, top_k=k, namespace="b")] == [matches(w) for w in dense.query_batch(Q, top_k=k)], k
    ix.close()
    dense.close()


@pytest.mark.parametrize("k", [10, 300])
def test_a_hybrid_query_with_radix_equals_the_one_with_rounds(idxmod, cuda, k):
    n, W = 1200, 4
    X, Q = data(n, 64, 61)
    rng = np.random.default_rng(7)
    dev = make_dev(idxmod, cuda, X, "float16", "dotproduct", select="rounds")
    dev.sparse_enable(W)
    dev.sparse_write(np.arange(n), [{"indices": rng.choice(16, W, replace=False).tolist(), "values": rng.standard_normal(W).tolist()}
                                    for _ in range(n)])
    q, sp = torch.from_numpy(Q[:1]), [{"indices": list(range(8)), "values": rng.standard_normal(8).tolist()}]
    want = run(dev.search_hybrid, q, k, n, sp)
    dev.set_deep_select("radix")
    got = run(dev.search_hybrid, q, k, n, sp)
    assert_same(got, want)
    assert_same((got[0][0], got[1][0]), reference(dev.scores_hybrid(q[0], n, sp[0]).cpu().numpy(), k))
    dev.close()


@pytest.mark.parametrize("dtype,metric,dim", FORMS)
def test_radix_and_rounds_return_the_same_bits(idxmod, cuda, dtype, metric, dim):
    n = 3001
    X, Q = data(n, dim, 3)
    dev = make_dev(idxmod, cuda, X, dtype, metric, select="rounds")
    want = run(dev.search_deep, torch.from_numpy(Q), 777, n)
    dev.set_deep_select("radix")
    assert_same(run(dev.search_deep, torch.from_numpy(Q), 777, n), want)
    dev.close()
    res = []
    for select in ("rounds", "radix"):
        ix = idxmod.Index("radix-pub", dimension=dim, metric=metric, dtype=dtype, capacity=n, device=cuda, max_top_k=1000, deep_select=select)
        ix.upsert_tensor([f"v{i}" for i in range(n)], torch.from_numpy(X).cuda())
        res.append(matches(ix.query(vector=Q[0].tolist(), top_k=1000)))
        ix.close()
    assert len(res[0]) == 1000 and res[0] == res[1]


def test_a_repeated_radix_call_allocates_nothing(idxmod, cuda):
    n = 3000
    X, Q = data(n, 64, 81)
    lib = import_pkg("_lib").load()
    dev = make_dev(idxmod, cuda, X, "float16")
    q = torch.from_numpy(Q).cuda()
    first = run(dev.search_deep, q, 1000, n)
    before = lib.rc_alloc_count()
    again = run(dev.search_deep, q, 1000, n)
    run(dev.search_deep, q[:2], 513, n)  # smaller calls fit the same workspace
    assert lib.rc_alloc_count() == before
    assert_same(again, first)
    dev.close()
