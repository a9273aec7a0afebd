"""GPU tests of the batched MFMA search over pages (``rc_index_search_pages_ex`` /
``rc_sharded_search_pages_ex``, through ``DeviceIndex.search_pages(mode=...)`` and
``ShardSet.search_pages(mode=...)``).

A namespace lies on a SHUFFLED page list inside a larger pool.  Every pool row that is not one of
its positions — every other page, and the tail of its last page at or past ``n_pos`` — holds a copy
of one of the queries, written before the namespace's rows: a path that scores one stale row shows
it as a top hit.  Every paged MFMA result must equal, scores and rows under ``torch.equal``,
  (a) the paged scan of the same slot, and
  (b) a dense index of the same vectors in position order searched with the same MFMA mode.
"""
import numpy as np
import pytest

from conftest import import_pkg

pytestmark = pytest.mark.gpu

PAGE = 256
SPARE_PAGES = 6
TWO_STAGES = 4096 + 3 * 256 + 77  # BATCH_CAND_CAP = 4096: a second stage, and a partial last page
THREE_STAGES = 70_001            # at k = 100 the stage ratio is 16: 4096, 65 536, 70 001


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


def pack(flags):
    return import_pkg("metafilter").pack_bits(np.asarray(flags, dtype=bool))


_DATA = {}


def data(n, dim, nq, seed, norms=False):
    """Vectors and queries, computed once per shape and left unchanged.  ``norms``: row norms spread
    over 0.25 .. 4 (the metric forms read them)."""
    key = (n, dim, nq, seed, norms)
    if key not in _DATA:
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((n, dim)).astype(np.float32)
        if norms:
            X *= (2.0 ** rng.uniform(-2.0, 2.0, n) / np.linalg.norm(X, axis=1)).astype(np.float32)[:, None]
        _DATA[key] = (X, rng.standard_normal((nq, dim)).astype(np.float32))
    return _DATA[key]


def local_rows(page_list, n):
    p = np.arange(n)
    return np.asarray(page_list, dtype=np.int64)[p // PAGE] * PAGE + p % PAGE


class Pair:
    """A dense DeviceIndex holding X in row order, and a pool holding X as slot 3 on a shuffled page
    list among decoys."""

    def __init__(self, idxmod, cuda, X, Q, dtype, metric="cosine", filt="native", seed=1):
        import torch

        n, dim = X.shape
        self.n, self.slot = n, 3
        n_pages = max(1, -(-n // PAGE))
        pool_pages = n_pages + SPARE_PAGES
        self.page_list = np.random.default_rng(seed).permutation(pool_pages)[:n_pages].tolist()
        self.dense = idxmod.DeviceIndex(dim, dtype=dtype, capacity=max(n, 1), device=cuda, metric=metric)
        self.pool = idxmod.DeviceIndex(dim, dtype=dtype, capacity=pool_pages * PAGE, device=cuda, metric=metric)
        if filt != "native":
            self.dense.set_filter(filt)
            self.pool.set_filter(filt)
        total = pool_pages * PAGE
        self.pool.upsert_rows(torch.from_numpy(Q[np.arange(total) % Q.shape[0]]), torch.arange(total))  # decoys everywhere
        if n:
            self.dense.upsert_rows(torch.from_numpy(X), torch.arange(n))
            self.pool.upsert_rows(torch.from_numpy(X), torch.from_numpy(local_rows(self.page_list, n)))
        self.pool.set_pages(self.slot, self.page_list)

    def check(self, q, k, mode="mfma", mask=None, what=None):
        """The paged MFMA search against both references; returns (scores, positions)."""
        import torch

        m = None if mask is None else torch.from_numpy(np.asarray(mask).view(np.int32)).to(self.pool.device)
        s0, r0 = self.pool.search_pages(q, k, self.slot, self.n, mask=m, mode="scan")
        s1, r1 = self.pool.search_pages(q, k, self.slot, self.n, mask=m, mode=mode)
        s2, r2 = self.dense.search(q, k, self.n, mode=mode, mask=m)
        torch.cuda.synchronize()
        assert torch.equal(s1, s0) and torch.equal(r1, r0), ("paged scan", what)
        assert torch.equal(s1, s2) and torch.equal(r1, r2), ("dense mfma", what)
        return s1.cpu().numpy(), r1.cpu().numpy()

    def close(self):
        self.dense.close()
        self.pool.close()


# (dtype, dim, n_pos, nq, k): every kernel form (ld 64 and 768: filter_gemm; ld 128 / 256 / 512:
# filter_qs NKT 2 / 4 / 8), each dtype, one / two / three stages, a padded width (dim 100), one padded
# query block (nq 9) and two query blocks (nq 300)
SHAPES = [
    ("float16", 512, 200, 9, 10),
    ("bfloat16", 256, TWO_STAGES, 9, 10),
    ("float16", 128, THREE_STAGES, 300, 100),
    ("bfloat16", 64, TWO_STAGES, 9, 10),
    ("float16", 768, THREE_STAGES, 9, 100),
    ("float16", 100, TWO_STAGES, 300, 10),
    ("bfloat16", 512, THREE_STAGES, 9, 100),
    ("float16", 64, THREE_STAGES, 300, 100),
]


@pytest.mark.parametrize("dtype,dim,n,nq,k", SHAPES)
def test_paged_mfma_equals_the_paged_scan_and_the_dense_mfma(idxmod, cuda, dtype, dim, n, nq, k):
    import torch

    X, Q = data(n, dim, nq, 11)
    pair = Pair(idxmod, cuda, X, Q, dtype)
    s, r = pair.check(torch.from_numpy(Q), k, what=(dtype, dim, n, nq, k))
    live = min(k, n)
    assert (r[:, :live] >= 0).all() and (r[:, :live] < n).all()
    if n == 200:  # k larger than n_pos: (-inf, -1) tails
        s, r = pair.check(torch.from_numpy(Q), 256, what="k > n_pos")
        assert (r[:, :n] >= 0).all() and (r[:, n:] == -1).all() and np.isneginf(s[:, n:]).all()
    pair.close()


@pytest.mark.parametrize("metric,masked", [("cosine", False), ("cosine", True), ("dotproduct", False), ("euclidean", True)])
def test_candidate_overflow_falls_back_to_the_paged_scan_exactly(idxmod, cuda, metric, masked):
    """Rows drawn from 3 directions: past the first stage every direction has more than twice the
    candidate capacity in exact ties, so the lists overflow and the flagged queries are re-run by the
    paged fallback scan on the device; ties still order by position."""
    import torch

    rng = np.random.default_rng(3)
    dim, n = 512, 48_000
    base = rng.standard_normal((3, dim)).astype(np.float32)
    pick = rng.integers(0, 3, n)
    flags = rng.random(n) < 0.75 if masked else np.ones(n, bool)
    for d in range(3):
        assert ((pick[4096:] == d) & flags[4096:]).sum() > 2 * 4096
    X = base[pick]
    Q = np.concatenate([base[:2], rng.standard_normal((14, dim)).astype(np.float32)])
    pair = Pair(idxmod, cuda, X, Q, "float16", metric, "metric" if metric != "cosine" else "native")
    pair.pool.timing(True)
    pair.pool.gemm_timing_read()
    m = torch.from_numpy(pack(flags).view(np.int32)).to(pair.pool.device) if masked else None
    s1, r1 = pair.pool.search_pages(torch.from_numpy(Q), 50, pair.slot, n, mask=m, mode="mfma")
    fallbacks = pair.pool.gemm_timing_read()[3]
    pair.pool.timing(False)
    s0, r0 = pair.pool.search_pages(torch.from_numpy(Q), 50, pair.slot, n, mask=m, mode="scan")
    torch.cuda.synchronize()
    assert fallbacks >= 1
    assert torch.equal(s1, s0) and torch.equal(r1, r0)
    first = np.nonzero((pick == 0) & flags)[0][:50]
    assert r1[0].cpu().numpy().tolist() == first.tolist()
    pair.close()


@pytest.mark.parametrize("dtype,dim,n,nq,k", [("float16", 512, THREE_STAGES, 9, 100), ("bfloat16", 768, TWO_STAGES, 9, 10),
                                              ("float16", 128, TWO_STAGES, 300, 10), ("bfloat16", 256, TWO_STAGES, 9, 10)])
def test_masked_paged_mfma_equals_the_masked_paged_scan(idxmod, cuda, dtype, dim, n, nq, k):
    import torch

    X, Q = data(n, dim, nq, 13)
    pair = Pair(idxmod, cuda, X, Q, dtype)
    rng = np.random.default_rng(5)
    n_pages = -(-n // PAGE)
    half = rng.random(n) < 0.5
    clustered = np.zeros(n, bool)  # ~1 % of the positions, in whole pages
    for p in rng.choice(n_pages - 1, max(1, n_pages // 100), replace=False):
        clustered[p * PAGE:(p + 1) * PAGE] = True
    gaps = half.copy()  # no eligible position in some pages, the last (partial) one among them
    for p in list(rng.choice(n_pages - 1, max(2, n_pages // 4), replace=False)) + [n_pages - 1]:
        gaps[p * PAGE:(p + 1) * PAGE] = False
    none = np.zeros(n, bool)
    for name, flags in (("half", half), ("clustered", clustered), ("gaps", gaps), ("none", none)):
        mask = pack(flags)
        for mode in ("mfma", "mfma_masked"):
            s, r = pair.check(torch.from_numpy(Q), k, mode=mode, mask=mask, what=(name, mode))
            assert flags[r[r >= 0]].all(), (name, mode)
            if name == "none":
                assert (r == -1).all() and np.isneginf(s).all()
    pair.close()


@pytest.mark.parametrize("dtype,dim,n,nq,k,metric", [("float16", 512, THREE_STAGES, 9, 100, "dotproduct"),
                                                     ("bfloat16", 64, TWO_STAGES, 9, 10, "euclidean"),
                                                     ("float16", 256, TWO_STAGES, 300, 10, "euclidean"),
                                                     ("bfloat16", 128, TWO_STAGES, 9, 10, "dotproduct"),
                                                     ("float16", 768, 200, 9, 10, "euclidean")])
def test_metric_paged_mfma_equals_the_paged_metric_scan(idxmod, cuda, dtype, dim, n, nq, k, metric):
    import torch

    X, Q = data(n, dim, nq, 17, norms=True)
    pair = Pair(idxmod, cuda, X, Q, dtype, metric, "metric")
    pair.check(torch.from_numpy(Q), k, what=(metric, "unmasked"))
    half = np.random.default_rng(9).random(n) < 0.5
    for mode in ("mfma", "mfma_masked"):  # the METRIC + MASKED forms
        if mode == "mfma_masked" and dim == 512:  # the one form that is not built (it would need scratch): refused
            m = torch.from_numpy(pack(half).view(np.int32)).to(pair.pool.device)
            with pytest.raises(ValueError) as e:
                pair.pool.search_pages(torch.from_numpy(Q), k, pair.slot, n, mask=m, mode=mode)
            assert e.value.code == import_pkg("_lib").RC_ERR_UNSUPPORTED
            pair.check(torch.from_numpy(Q), k, mode=mode, what="without a mask it is mfma")
            continue
        s, r = pair.check(torch.from_numpy(Q), k, mode=mode, mask=pack(half), what=(metric, mode))
        assert half[r[r >= 0]].all()
    pair.close()


@pytest.mark.parametrize("remote", [False, True])
def test_two_shards_on_one_gpu(idxmod, cuda, remote):
    """ShardSet.search_pages(mode="mfma") on two shards (with and without the cross-device path)
    against the dense two-shard set and the paged scan; n_pos = 1 leaves shard 1 with no position."""
    import torch

    pages = import_pkg("pages")
    S, dim, nq = 2, 512, 9
    for n, k in ((2 * TWO_STAGES + 1, 10), (1, 5)):
        X, Q = data(n, dim, nq, 23)
        dense = idxmod.ShardSet(dim, dtype="float16", capacity_per_shard=-(-n // S) + 1, devices=[cuda] * S)
        n_pages = pages.pages_for(n, S)
        pool_pages = n_pages + SPARE_PAGES
        pool = idxmod.ShardSet(dim, dtype="float16", capacity_per_shard=pool_pages * PAGE, devices=[cuda] * S)
        if remote:
            dense.force_remote()
            pool.force_remote()
        page_list = np.random.default_rng(4).permutation(pool_pages)[:n_pages].tolist()
        total = pool_pages * PAGE * S
        pool.upsert_rows(torch.from_numpy(Q[np.arange(total) % nq]), np.arange(total))
        dense.upsert_rows(torch.from_numpy(X), np.arange(n))
        pool.upsert_rows(torch.from_numpy(X), pages.positions_to_rows(page_list, range(n), S))
        pool.set_pages(3, page_list)
        q = torch.from_numpy(Q)
        half = np.random.default_rng(6).random(n) < 0.5
        for mode, mask in (("mfma", None), ("mfma_masked", pack(half)), ("auto", None)):
            s0, r0 = pool.search_pages(q, k, 3, n, mask=mask, mode="scan")
            s1, r1 = pool.search_pages(q, k, 3, n, mask=mask, mode=mode)
            s2, r2 = dense.search(q, k, n, mode="mfma" if mode == "auto" else mode, mask=mask)
            torch.cuda.synchronize()
            assert torch.equal(s1, s0) and torch.equal(r1, r0), (n, mode)
            assert torch.equal(s1, s2) and torch.equal(r1, r2), (n, mode)
        dense.close()
        pool.close()


def test_auto_takes_the_batched_path_without_a_mask_and_scans_with_one(idxmod, cuda):
    import torch

    dim, n, nq = 64, 263_000, 64
    pool = idxmod.DeviceIndex(dim, dtype="float16", capacity=(-(-n // PAGE) + SPARE_PAGES) * PAGE, device=cuda)
    pool.fill_random(9, 0, pool.capacity)
    page_list = np.random.default_rng(8).permutation(pool.capacity // PAGE)[:-(-n // PAGE)].tolist()
    pool.set_pages(0, page_list)
    q = torch.from_numpy(np.random.default_rng(2).standard_normal((nq, dim)).astype(np.float32))
    s0, r0 = pool.search_pages(q, 10, 0, n)
    mask = torch.from_numpy(pack(np.arange(n) % 2 == 0).view(np.int32)).to(pool.device)
    pool.timing(True)
    pool.gemm_timing_read()
    s1, r1 = pool.search_pages(q, 10, 0, n, mode="auto")
    launches = pool.gemm_timing_read()[1]
    s2, r2 = pool.search_pages(q[:16], 10, 0, n, mode="auto")  # 16 queries from 262 144 positions
    s3, r3 = pool.search_pages(q, 10, 0, 66_000, mode="auto")  # 64 queries from 65 536
    corners = pool.gemm_timing_read()[1]
    pool.search_pages(q, 10, 0, n, mode="auto", mask=mask)
    pool.search_pages(q[:15], 10, 0, n, mode="auto")      # too few queries
    pool.search_pages(q[:63], 10, 0, 262_000, mode="auto")  # too few queries for this many positions
    pool.search_pages(q, 10, 0, 65_000, mode="auto")      # too few positions
    scanned = pool.gemm_timing_read()[1]
    pool.timing(False)
    torch.cuda.synchronize()
    assert launches >= 1 and corners >= 2 and scanned == 0
    assert torch.equal(s2, s0[:16]) and torch.equal(r2, r0[:16])
    s4, r4 = pool.search_pages(q, 10, 0, 66_000)
    assert torch.equal(s3, s4) and torch.equal(r3, r4)
    assert torch.equal(s1, s0) and torch.equal(r1, r0)
    pool.close()


@pytest.mark.parametrize("dtype,metric,filt", [("float32", "cosine", "native"), ("float8_e4m3fn", "cosine", "native"),
                                               ("float16", "cosine", "i8"), ("float16", "dotproduct", "native")])
def test_pools_without_a_paged_form_refuse_mfma_and_scan_on_auto(idxmod, cuda, dtype, metric, filt):
    import torch

    lib = import_pkg("_lib")
    dim, n, nq = 256, 66_000, 64  # a shape at which "auto" takes the batched path where there is one
    pool = idxmod.DeviceIndex(dim, dtype=dtype, capacity=(-(-n // PAGE) + SPARE_PAGES) * PAGE, device=cuda, metric=metric)
    pool.fill_random(9, 0, pool.capacity)
    if filt != "native":
        pool.set_filter(filt)
    pool.set_pages(0, np.random.default_rng(8).permutation(pool.capacity // PAGE)[:-(-n // PAGE)].tolist())
    q = torch.from_numpy(np.random.default_rng(2).standard_normal((nq, dim)).astype(np.float32))
    for mode in ("mfma", "mfma_masked"):
        with pytest.raises(ValueError) as e:
            pool.search_pages(q, 10, 0, n, mode=mode)
        assert e.value.code == lib.RC_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="unknown search mode"):
        pool.search_pages(q, 10, 0, n, mode="fast")
    s0, r0 = pool.search_pages(q, 10, 0, n)
    s1, r1 = pool.search_pages(q, 10, 0, n, mode="auto")
    torch.cuda.synchronize()
    assert torch.equal(s1, s0) and torch.equal(r1, r0)
    pool.close()
