"""The search entry points against each other on one tiny corpus: what a mis-wired argument would
break (a slot taken for the rows, a dropped mask, the wrong k bound, a result written to the wrong
buffer) and a per-feature test could miss.  Every equality here is one the docstrings of
``index.py`` promise, and every one is bitwise.

The corpus: 600 f16 vectors (two full pages and a partial one on one shard) in the dense rows
[0, 600) of a dotproduct ShardSet and again, in position order, in a slot whose page list is not
the identity; a sparse store of width 4 in which every second record holds one or two entries;
one shard, and two shards of one device."""
import numpy as np
import pytest

from conftest import import_pkg

pytestmark = pytest.mark.gpu

N, DIM, NQ, K, SLOT, WIDTH = 600, 64, 3, 7, 2, 4
PAGE_LIST = [5, 3, 4]  # past the pages of the dense rows (0 .. 2), and not in order
VOCAB = [3, 17, 40, 99, 1000]


def corpus():
    rng = np.random.default_rng(1907)
    X = rng.standard_normal((N, DIM)).astype(np.float32)
    Q = rng.standard_normal((NQ, DIM)).astype(np.float32)
    sparse = [None] * N
    for r in range(0, N, 2):  # every second record: one or two entries
        idx = sorted(rng.choice(VOCAB, 1 + (r // 2) % 2, replace=False).tolist())
        sparse[r] = {"indices": idx, "values": [float(np.float32(v)) for v in rng.uniform(1.0, 4.0, len(idx))]}
    sq = [{"indices": [3, 40, 1000], "values": [2.0, -1.5, 3.0]}, {"indices": [17], "values": [4.0]},
          {"indices": [3, 17, 40, 99], "values": [1.0, 1.0, 1.0, 1.0]}]
    flags = np.arange(N) % 3 != 0  # clears every third row, the first among them
    flags[N - 1] = False           # ... and the last
    return X, Q, sparse, sq, flags


def np2(pair):
    """(score bits, rows) of a search result, device tensors or host arrays (copied: query_host reuses its own)."""
    s, r = pair[0], pair[1]
    if not isinstance(s, np.ndarray):
        s, r = s.cpu().numpy(), r.cpu().numpy()
    return np.array(s, np.float32).view(np.uint32).copy(), np.array(r, np.int64)


def run(ss, X, Q, sparse, sq, mask):
    """Every search form of one ShardSet over the corpus, by name."""
    import torch

    q = torch.from_numpy(Q)
    out = {
        "search": ss.search(q, K, N, mode="scan", mask=mask),
        "search_pages": ss.search_pages(q, K, SLOT, N, mask=mask, mode="scan"),
        "search_deep": ss.search_deep(q, K, N, mask=mask),
        "search_pages_deep": ss.search_pages_deep(q, K, SLOT, N, mask=mask),
        "search_hybrid(None)": ss.search_hybrid(q, K, N, [None] * NQ, mask=mask),
        "search_hybrid": ss.search_hybrid(q, K, N, sq, mask=mask),
        "search_pages_hybrid": ss.search_pages_hybrid(q, K, SLOT, N, sq, mask=mask),
    }
    torch.cuda.synchronize()
    out = {name: np2(res) for name, res in out.items()}
    out["query_host"] = np2(ss.query_host(Q, K, N, False, mask=mask))
    out["query_host_pages"] = np2(ss.query_host_pages(Q, K, SLOT, N, False, mask=mask))
    return out


def same(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what


@pytest.fixture(scope="module")
def results(cuda):
    """{shards: {masked: {entry point: (score bits, rows)}}} and the hybrid score arrays, computed once."""
    import torch

    idxmod, pages = import_pkg("index"), import_pkg("pages")
    X, Q, sparse, sq, flags = corpus()
    mask = import_pkg("metafilter").pack_bits(flags)
    res, scores = {}, {}
    for S in (1, 2):
        ss = idxmod.ShardSet(DIM, dtype="float16", capacity_per_shard=6 * 256, devices=[cuda] * S, metric="dotproduct")
        try:
            ss.sparse_enable(WIDTH)
            page_list = PAGE_LIST[:pages.pages_for(N, S)]
            for rows in (list(range(N)), pages.positions_to_rows(page_list, range(N), S)):
                ss.upsert_rows(torch.from_numpy(X), np.asarray(rows))
                ss.sparse_write(rows, sparse)
            ss.set_pages(SLOT, page_list)
            res[S] = {masked: run(ss, X, Q, sparse, sq, mask if masked else None) for masked in (False, True)}
            q0 = torch.from_numpy(Q[:1])
            scores[S] = (ss.scores_hybrid(q0, N, sq[0]).cpu().numpy().view(np.uint32),
                         ss.scores_hybrid(q0, N, sq[0], slot=SLOT).cpu().numpy().view(np.uint32))
        finally:
            ss.close()
    return res, scores, flags


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("S", [1, 2])
def test_entry_points_agree(results, S, masked):
    r = results[0][S][masked]
    same(r["search_pages"], r["search"], "search_pages(scan) = search(scan)")
    same(r["search_deep"], r["search"], "search_deep = search(scan)")
    same(r["search_pages_deep"], r["search_deep"], "search_pages_deep = search_deep")
    same(r["search_hybrid(None)"], r["search_deep"], "search_hybrid without sparse parts = search_deep")
    same(r["search_pages_hybrid"], r["search_hybrid"], "search_pages_hybrid = search_hybrid")
    same(r["query_host"], r["search"], "query_host = search(scan)")
    same(r["query_host_pages"], r["search"], "query_host_pages = search(scan)")
    # the comparisons above compare something: the sparse parts move the scores, the lists are full
    assert not np.array_equal(r["search_hybrid"][0], r["search_deep"][0])
    assert all((res[1] >= 0).all() and (res[1] < N).all() for res in r.values())


@pytest.mark.parametrize("masked", [False, True])
def test_two_shards_equal_one(results, masked):
    one, two = results[0][1][masked], results[0][2][masked]
    assert one.keys() == two.keys()
    for name in one:
        same(two[name], one[name], name)


@pytest.mark.parametrize("S", [1, 2])
def test_the_mask_reaches_every_entry_point(results, S):
    res, _, flags = results
    for name, (_, rows) in res[S][True].items():
        assert flags[rows].all(), name  # no cleared row comes back
        assert not np.array_equal(rows, res[S][False][name][1]), name  # and the mask changed the answer


def test_scores_hybrid_over_a_slot(results):
    _, scores, _ = results
    for S in (1, 2):
        assert np.array_equal(scores[S][1], scores[S][0]), S
    assert np.array_equal(scores[2][0], scores[1][0])
