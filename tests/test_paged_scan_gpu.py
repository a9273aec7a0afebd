"""GPU tests of the page-table scan (``rc_sharded_search_pages`` / ``rc_index_search_pages``,
through ``ShardSet``): a namespace's vectors on a non-monotonic page list inside a pool full of
decoys must give the scores (bit for bit), positions and tie order of a dense ``ShardSet`` with
the same shard count holding the same vectors in position order, searched with ``mode="scan"``.

Every pool row that is not one of the namespace's — every other page, and the unused tail of its
last page — holds a copy of one of the queries, written before the namespace's rows: a row scored
from the wrong page, or past the count, ranks first.
"""
import numpy as np
import pytest

from conftest import import_pkg

pytestmark = pytest.mark.gpu

PAGE = 256
PAGE_LIST = [5, 2, 9, 0, 7]
POOL_PAGES = 10
NQ = 9


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


@pytest.fixture(scope="module")
def pages(cuda):
    return import_pkg("pages")


def pack(flags):
    return import_pkg("metafilter").pack_bits(np.asarray(flags, dtype=bool))


_DATA = {}


def data(n, dim, seed):
    """Vectors and queries, computed once per shape and left unchanged."""
    key = (n, dim, seed)
    if key not in _DATA:
        rng = np.random.default_rng(seed)
        _DATA[key] = (rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((NQ, dim)).astype(np.float32))
    return _DATA[key]


def bits(a):
    return a.cpu().numpy().view(np.int32)


class Pair:
    """A dense ShardSet holding X in row order and a pool holding X as slot 3 on PAGE_LIST."""

    def __init__(self, idxmod, pages, cuda, X, Q, S, dtype="float32", metric="cosine", remote=False, page_list=PAGE_LIST):
        import torch

        n, dim = X.shape
        self.n, self.S, self.slot = n, S, 3
        self.dense = idxmod.ShardSet(dim, dtype=dtype, capacity_per_shard=-(-n // S) + 1, devices=[cuda] * S, metric=metric)
        self.pool = idxmod.ShardSet(dim, dtype=dtype, capacity_per_shard=POOL_PAGES * PAGE, devices=[cuda] * S, metric=metric)
        if remote:
            self.dense.force_remote()
            self.pool.force_remote()
        self.dense.upsert_rows(torch.from_numpy(X), np.arange(n))
        total = POOL_PAGES * PAGE * S
        self.pool.upsert_rows(torch.from_numpy(Q[np.arange(total) % Q.shape[0]]), np.arange(total))  # decoys everywhere
        self.page_list = list(page_list[:pages.pages_for(n, S)])
        self.pool.upsert_rows(torch.from_numpy(X), pages.positions_to_rows(self.page_list, range(n), S))
        self.pool.set_pages(self.slot, self.page_list)

    def check(self, q, k, mask=None, what=None):
        import torch

        s0, r0 = self.dense.search(q, k, self.n, mode="scan", mask=mask)
        s1, r1 = self.pool.search_pages(q, k, self.slot, self.n, mask=mask)
        torch.cuda.synchronize()
        assert np.array_equal(bits(s0), bits(s1)), what
        assert np.array_equal(r0.cpu().numpy(), r1.cpu().numpy()), what
        return s1.cpu().numpy(), r1.cpu().numpy()

    def close(self):
        self.dense.close()
        self.pool.close()


def edge_counts(S):
    return sorted({1, 255, 256, 257, 256 * S - 1, 256 * S, 256 * S + 1, 3 * 256 * S + 77})


# every n at both shard counts; the dtypes, widths and metrics cycle over the cases, so that each
# value occurs (and each dtype meets each metric form at least once across the two lists)
CASES = []
_KINDS = [("float32", 512, "cosine"), ("float16", 64, "cosine"), ("bfloat16", 768, "dotproduct"), ("float8_e4m3fn", 512, "cosine"),
          ("float16", 768, "euclidean"), ("float32", 64, "dotproduct"), ("bfloat16", 512, "cosine"), ("float8_e4m3fn", 64, "euclidean"),
          ("float32", 768, "cosine")]
for _S in (1, 3):
    for _i, _n in enumerate(edge_counts(_S)):
        _dt, _dim, _metric = _KINDS[(_i + 4 * (_S == 3)) % len(_KINDS)]
        CASES.append((_S, _S == 3 and _i % 3 == 1, _n, _dt, _dim, _metric))


@pytest.mark.parametrize("S,remote,n,dtype,dim,metric", CASES)
def test_paged_scan_equals_the_dense_scan_bit_for_bit(idxmod, pages, cuda, S, remote, n, dtype, dim, metric):
    import torch

    X, Q = data(n, dim, 7)
    pair = Pair(idxmod, pages, cuda, X, Q, S, dtype, metric, remote)
    for nq in (1, 2, 5, 9):  # 1-, 2- and 4-query passes and the zero-padded slot (by row width and k)
        q = torch.from_numpy(Q[:nq])
        for k in (1, 10, 100, 256):
            s, r = pair.check(q, k, what=(nq, k))
            live = min(k, n)
            assert (r[:, :live] >= 0).all() and (r[:, :live] < n).all()
            assert (r[:, live:] == -1).all() and np.isneginf(s[:, live:]).all()  # k > n: (-inf, -1) padding
    pair.close()


@pytest.mark.parametrize("S", [1, 3])
def test_ties_order_by_position_across_descending_pages(idxmod, pages, cuda, S):
    """Duplicates on different pages whose page numbers descend (5, then 2) while their positions
    ascend: equal scores come back in ascending position, as the dense index orders them."""
    import torch

    n = 3 * 256 * S + 77
    X, Q = data(n, 512, 3)
    X, Q = X.copy(), Q.copy()
    span = 256 * S
    dup = [7, span + 3, span + 4, 2 * span + 250, 3 * span + 70]  # list pages 0, 1, 1, 2, 3 = pool pages 5, 2, 2, 9, 0
    X[dup] = X[dup[0]]
    Q[0] = X[dup[0]]
    pair = Pair(idxmod, pages, cuda, X, Q, S, "float16")
    s, r = pair.check(torch.from_numpy(Q[:2]), 10, what="ties")
    assert r[0, :len(dup)].tolist() == dup
    assert len(set(s[0, :len(dup)].tolist())) == 1
    pair.close()


@pytest.mark.parametrize("S,dtype,dim,metric", [(1, "float16", 512, "cosine"), (3, "float32", 768, "euclidean"),
                                                (3, "float8_e4m3fn", 64, "cosine"), (1, "bfloat16", 64, "dotproduct")])
def test_masked_paged_scan_equals_the_dense_masked_scan(idxmod, pages, cuda, S, dtype, dim, metric):
    import torch

    n = 3 * 256 * S + 77
    X, Q = data(n, dim, 13)
    pair = Pair(idxmod, pages, cuda, X, Q, S, dtype, metric, remote=(S == 3))
    rng = np.random.default_rng(5)
    share = rng.random(n) < 0.3
    holes = share.copy()
    for b0 in (0, 64, 248, 256 * S, n - 80):  # whole zero bytes (8 aligned positions), also across a page edge
        holes[b0:b0 + 24] = False
    one = np.zeros(n, bool)
    one[n - 5] = True  # a single bit, in the last, partial page
    none = np.zeros(n, bool)
    for name, flags in (("share", share), ("zero-bytes", holes), ("one-bit", one), ("empty", none)):
        mask = pack(flags)
        for nq, k in ((1, 10), (5, 10), (2, 64), (1, 100), (9, 256)):
            s, r = pair.check(torch.from_numpy(Q[:nq]), k, mask=mask, what=(name, nq, k))
            got = r[r >= 0]
            assert flags[got].all(), name
            if name == "one-bit":
                assert (r[:, 0] == n - 5).all() and (r[:, 1:] == -1).all()
            if name == "empty":
                assert (r == -1).all() and np.isneginf(s).all()
    pair.close()


def test_reused_pages_never_show_their_old_rows(idxmod, pages, cuda):
    """A namespace's pages go to a shorter one: what the old one left past the new count (copies
    of the query, so they would rank first) never appears."""
    import torch

    S, dim, n_old, n_new = 3, 512, 3 * 256 * 3 + 77, 256 * 3 + 40
    Xn, Q = data(n_new, dim, 21)
    rng = np.random.default_rng(2)
    old = (Q[0][None] + 1e-3 * rng.standard_normal((n_old, dim))).astype(np.float32)
    pair = Pair(idxmod, pages, cuda, old, Q, S, "float32")
    pair.pool.set_pages(pair.slot, [])  # the old namespace is gone; its pages are free
    with pytest.raises(ValueError):
        pair.pool.search_pages(torch.from_numpy(Q[:1]), 5, pair.slot, 1)
    new_list = pair.page_list[:pages.pages_for(n_new, S)]
    pair.pool.upsert_rows(torch.from_numpy(Xn), pages.positions_to_rows(new_list, range(n_new), S))
    pair.pool.set_pages(8, new_list)
    dense = idxmod.ShardSet(dim, capacity_per_shard=-(-n_new // S) + 1, devices=[cuda] * S)
    dense.upsert_rows(torch.from_numpy(Xn), np.arange(n_new))
    for k in (10, 256):
        s0, r0 = dense.search(torch.from_numpy(Q[:5]), k, n_new, mode="scan")
        s1, r1 = pair.pool.search_pages(torch.from_numpy(Q[:5]), k, 8, n_new)
        torch.cuda.synchronize()
        assert np.array_equal(bits(s0), bits(s1)) and np.array_equal(r0.cpu().numpy(), r1.cpu().numpy())
        assert (r1.cpu().numpy() < n_new).all()
    dense.close()
    pair.close()


@pytest.mark.parametrize("S", [1, 3])
def test_query_host_pages_returns_positions_and_their_values(idxmod, pages, cuda, S):
    """The request path over a slot: the lists of search_pages, and each matched position's
    values gathered through the page table (what fetch gives for its pool row)."""
    import torch

    n = 256 * S + 1
    X, Q = data(n, 768, 31)
    pair = Pair(idxmod, pages, cuda, X, Q, S, "float32")
    mask = pack(np.arange(n) % 3 == 0)
    for nq, k, m in ((1, 5, None), (3, 256, None), (2, 10, mask)):
        s1, r1 = pair.pool.search_pages(torch.from_numpy(Q[:nq]), k, pair.slot, n, mask=m)
        torch.cuda.synchronize()
        sc, rw, val = pair.pool.query_host_pages(np.ascontiguousarray(Q[:nq]), k, pair.slot, n, True, mask=m)
        assert np.array_equal(sc.view(np.int32), bits(s1)) and np.array_equal(rw, r1.cpu().numpy())
        for qi in range(nq):
            live = rw[qi] >= 0
            want = pair.pool.fetch_rows(pages.positions_to_rows(pair.page_list, rw[qi][live], S)).numpy()
            assert np.array_equal(val[qi][live], want)
            assert np.isnan(val[qi][~live]).all()
        sc2, rw2, none = pair.pool.query_host_pages(np.ascontiguousarray(Q[:nq]), k, pair.slot, n, False, mask=m)
        assert none is None and np.array_equal(rw2, rw) and np.array_equal(sc2.view(np.int32), sc.view(np.int32))
    pair.close()


def test_paged_calls_check_their_arguments(idxmod, cuda):
    import torch

    S, dim = 3, 64
    pool = idxmod.ShardSet(dim, capacity_per_shard=4 * PAGE, devices=[cuda] * S)
    q = torch.zeros((1, dim)) + 1.0
    with pytest.raises(ValueError, match="unknown slot"):
        pool.search_pages(q, 5, 0, 1)
    with pytest.raises(ValueError, match="capacity"):
        pool.set_pages(0, [1, 4])  # 4 pages per shard: page 4 is past them
    with pytest.raises(ValueError, match="unknown slot"):
        pool.search_pages(q, 5, 0, 1)  # the refused call installed nothing
    pool.set_pages(0, [3, 1])
    with pytest.raises(ValueError, match="n_pos"):
        pool.search_pages(q, 5, 0, 2 * PAGE * S + 1)
    with pytest.raises(ValueError, match="top_k"):
        pool.search_pages(q, 257, 0, 10)
    with pytest.raises(ValueError, match="unknown slot"):
        pool.query_host_pages(np.ones((1, dim), np.float32), 5, 1, 10, True)
    s, r = pool.search_pages(q, 5, 0, 2 * PAGE * S)  # exactly the pages' rows: accepted
    torch.cuda.synchronize()
    assert s.shape == (1, 5)
    pool.grow(8 * PAGE)
    pool.set_pages(0, [3, 1, 7])  # after growth page 7 exists
    pool.close()
