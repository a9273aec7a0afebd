"""GPU tests of the row-masked exact search (``rc_index_search_masked`` and the sharded /
``Index``-level forms built on it): Pinecone's ``index.query(..., filter={...})``.

The masked oracle lives here: ``oracle.cosine_topk.cosine_topk`` on the eligible subset of the
STORED rows, row numbers mapped back.  Where a case fits one unmasked search (``n_rows <= 256``)
the check is stronger: the device's own total order, filtered by the mask, bit for bit.
"""
import numpy as np
import pytest

from conftest import import_pkg
from oracle.cosine_topk import cosine_topk, topk_equal_modulo_ties

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float16", "bfloat16"]


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


def search_masked(L, dev, q, k, n_rows, mask, mode="scan"):
    """rc_index_search_masked itself (mask: device int32 tensor or None = NULL)."""
    import torch

    lib = L.load()
    q = q.to(device=dev.device, dtype=torch.float32).contiguous()
    s = torch.empty((q.shape[0], k), dtype=torch.float32, device=dev.device)
    r = torch.empty((q.shape[0], k), dtype=torch.int64, device=dev.device)
    L.check(lib.rc_index_search_masked(dev.handle, L.ptr(q), q.shape[0], int(n_rows), int(k), L.ptr(mask), L.ptr(s), L.ptr(r),
                                       L.SEARCH_MODES[mode], L.stream_ptr(None)))
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


_DATA = {}


def data(n, dim, nq, seed):
    """Rows and queries, computed once per shape and left unchanged."""
    key = (n, dim, nq, seed)
    if key not in _DATA:
        rng = np.random.default_rng(seed)
        _DATA[key] = (rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((nq, dim)).astype(np.float32))
    return _DATA[key]


def make_index(idxmod, cuda, X, dtype):
    import torch

    dev = idxmod.DeviceIndex(X.shape[1], dtype=dtype, capacity=X.shape[0] + 3, device=cuda)
    dev.upsert_rows(torch.from_numpy(X), torch.arange(X.shape[0], dtype=torch.int64))
    return dev


def expect_from_order(order_s, order_r, flags, k):
    """The device's total order (one query) filtered by the mask, padded with (-inf, -1)."""
    keep = [j for j, r in enumerate(order_r) if r >= 0 and flags[r]][:k]
    s = np.full(k, -np.inf, np.float32)
    r = np.full(k, -1, np.int64)
    s[:len(keep)] = order_s[keep]
    r[:len(keep)] = order_r[keep]
    return s, r


# ------------------------------------------------------------------ identity --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [128, 512, 768])  # 4, 2 and 1 queries per scan pass
def test_all_ones_and_null_mask_equal_the_unmasked_search(idxmod, L, cuda, dtype, dim):
    import torch

    n = 3001  # several blocks and a ragged tail
    X, Q = data(n, dim, 5, 11)
    dev = make_index(idxmod, cuda, X, dtype)
    ones = dev_mask(np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32), dev.device)
    for nq in (1, 3, 5):
        q = torch.from_numpy(Q[:nq])
        for k in (1, 10, 130, 256):
            s0, r0 = dev.search(q, k, n, mode="scan")
            torch.cuda.synchronize()
            s0, r0 = s0.cpu().numpy(), r0.cpu().numpy()
            for mask in (ones, None):
                s1, r1 = search_masked(L, dev, q, k, n, mask)
                assert same_bits(s0, s1) and np.array_equal(r0, r1), (nq, k, mask is None)
    dev.close()


# ------------------------------------------- exact order on the device's scores --
@pytest.mark.parametrize("dtype,dim", [("float32", 512), ("float16", 128), ("bfloat16", 768)])
def test_masked_topk_is_the_devices_order_filtered(idxmod, L, cuda, dtype, dim):
    import torch

    n = 200
    X, Q = data(n, dim, 3, 5)
    X = X.copy()
    X[60:70] = X[60]  # duplicates straddling a mask word boundary and eligible / ineligible rows
    Q = Q.copy()
    Q[0] = X[60] + 0.05 * Q[0]
    dev = make_index(idxmod, cuda, X, dtype)
    q = torch.from_numpy(Q)
    full_s, full_r = search_masked(L, dev, q, n, n, None)
    assert all(sorted(full_r[qi].tolist()) == list(range(n)) for qi in range(3))
    assert full_r[0, :10].tolist() == list(range(60, 70))  # the ties, row ascending
    rng = np.random.default_rng(17)
    flags = rng.random(n) < 0.5
    flags[60:70] = [False, True, False, True, True, False, False, True, False, False]
    for k in (1, 10, 200):
        s, r = search_masked(L, dev, q, k, n, dev_mask(pack(flags), dev.device))
        for qi in range(3):
            es, er = expect_from_order(full_s[qi], full_r[qi], flags, k)
            assert np.array_equal(r[qi], er) and same_bits(s[qi], es), (k, qi)
    assert search_masked(L, dev, q, 10, n, dev_mask(pack(flags), dev.device))[1][0, :4].tolist() == [61, 63, 64, 67]
    dev.close()


# --------------------------------------------------------------------- edges --
@pytest.mark.parametrize("n", [1, 31, 33])
def test_small_indexes_empty_masks_and_garbage_bits(idxmod, L, cuda, n):
    import torch

    X, Q = data(n, 512, 2, 23 + n)
    dev = make_index(idxmod, cuda, X, "float32")
    q = torch.from_numpy(Q)
    full_s, full_r = search_masked(L, dev, q, n, n, None)
    words = (n + 31) // 32
    # all zero: every slot empty
    s, r = search_masked(L, dev, q, 5, n, dev_mask(np.zeros(words, np.uint32), dev.device))
    assert np.all(r == -1) and np.all(np.isneginf(s))
    # fewer eligible rows than k, and garbage bits at and past n_rows (and a whole garbage word)
    flags = np.zeros(n, bool)
    flags[::3] = True
    bm = np.concatenate([pack(flags), np.zeros(1, np.uint32)])
    for w in range(bm.shape[0]):
        for b in range(32):
            if w * 32 + b >= n:
                bm[w] |= np.uint32(1 << b)
    for k in (1, 5, 40):
        s, r = search_masked(L, dev, q, k, n, dev_mask(bm, dev.device))
        for qi in range(2):
            es, er = expect_from_order(full_s[qi], full_r[qi], flags, k)
            assert np.array_equal(r[qi], er) and same_bits(s[qi], es), (k, qi)
    # garbage only: still nothing eligible
    only = bm.copy()
    only[:words] &= ~pack(np.ones(n, bool))
    s, r = search_masked(L, dev, q, 3, n, dev_mask(only, dev.device))
    assert np.all(r == -1) and np.all(np.isneginf(s))
    dev.close()


def _subset_oracle(Xs, Q, flags, k):
    el = np.nonzero(flags)[0]
    rr, ss = cosine_topk(Xs[el], Q, k, rows_normalized=True)
    return el[rr], ss


def _check_vs_oracle(Xs, Q, flags, k, s, r, unmasked=None, tol=1e-5):
    """Top-k equal to the subset oracle's modulo ties within tol (the bar tests/test_index_gpu.py
    sets for the unmasked search, every dtype: the oracle runs on the stored rows); every
    returned row eligible; scores those of the oracle for the returned rows, descending."""
    ref_r, ref_s = _subset_oracle(Xs, Q, flags, k)
    kk = ref_r.shape[1]
    for qi in range(Q.shape[0]):
        assert topk_equal_modulo_ties(r[qi, :kk], s[qi, :kk], ref_r[qi], ref_s[qi], tol), (qi, r[qi], ref_r[qi])
        assert np.all(flags[r[qi, :kk]])
        qn = Q[qi].astype(np.float64) / np.linalg.norm(Q[qi].astype(np.float64))
        assert np.allclose(s[qi, :kk], Xs[r[qi, :kk]].astype(np.float64) @ qn, atol=tol, rtol=0)
        assert np.all(np.diff(s[qi, :kk]) <= 0)
        assert np.all(r[qi, kk:] == -1) and np.all(np.isneginf(s[qi, kk:]))
        if unmasked is not None:  # a row both searches return has the same score bits
            us, ur = unmasked
            at = {int(row): j for j, row in enumerate(ur[qi])}
            for j in range(kk):
                if int(r[qi, j]) in at:
                    assert same_bits(s[qi, j], us[qi, at[int(r[qi, j])]])


def test_skip_branch_whole_groups_clear(idxmod, L, cuda):
    """1100 rows = 3 blocks of 384 / 384 / 332 rows.  Masks that clear whole 8-row and whole 32-row
    groups (the skip branch), and one whose only eligible rows sit in the last block's final,
    partial 8-row group (rows 1096 .. 1099)."""
    import torch

    n = 1100
    X, Q = data(n, 512, 3, 31)
    dev = make_index(idxmod, cuda, X, "float32")
    Xs = dev.stored_rows(n).cpu().numpy()
    q = torch.from_numpy(Q)
    un = search_masked(L, dev, q, 256, n, None)
    rows = np.arange(n)
    cases = {
        "8-row groups": (rows // 8) % 3 == 0,
        "32-row groups": (rows // 32) % 2 == 1,
        "mixed": ((rows // 32) % 4 != 0) & ((rows // 8) % 2 == 0) & (rows % 5 != 0),
        "one row per block": np.isin(rows, [383, 384, 1099]),
        "last partial group": rows >= 1096,
        "last partial group, two rows": np.isin(rows, [1097, 1099]),
    }
    for name, flags in cases.items():
        for k in (1, 10, 100):
            s, r = search_masked(L, dev, q, k, n, dev_mask(pack(flags), dev.device))
            _check_vs_oracle(Xs, Q, flags, k, s, r, unmasked=un)
    s, r = search_masked(L, dev, q, 10, n, dev_mask(pack(cases["last partial group, two rows"]), dev.device))
    assert all(sorted(r[qi, :2].tolist()) == [1097, 1099] and np.all(r[qi, 2:] == -1) for qi in range(3))
    dev.close()


# -------------------------------------------------------------------- oracle --
@pytest.mark.parametrize("dtype", DTYPES)
def test_masked_search_matches_the_subset_oracle(idxmod, L, cuda, dtype):
    import torch

    n = 10000
    X, Q = data(n, 512, 5, 41)
    dev = make_index(idxmod, cuda, X, dtype)
    Xs = dev.stored_rows(n).cpu().numpy()
    q = torch.from_numpy(Q)
    un = search_masked(L, dev, q, 256, n, None)
    rng = np.random.default_rng(43)
    for share in (0.5, 0.01):
        flags = rng.random(n) < share
        s, r = search_masked(L, dev, q, 10, n, dev_mask(pack(flags), dev.device))
        _check_vs_oracle(Xs, Q, flags, 10, s, r, unmasked=un)
    dev.close()


# ----------------------------------------------------------------- MFMA mode --
def test_mfma_mode_with_a_mask_equals_the_masked_scan(idxmod, L, cuda):
    import torch

    n = 20000
    X, Q = data(n, 256, 16, 51)
    dev = make_index(idxmod, cuda, X, "float16")
    q = torch.from_numpy(Q)
    rng = np.random.default_rng(53)
    half = rng.random(n) < 0.5
    tail = np.arange(n) >= 16384  # stage 1 (the first 4096 rows) sees no eligible row; stage 2 overflows
    dev.gemm_timing_read()
    for name, flags in (("half", half), ("tail", tail)):
        m = dev_mask(pack(flags), dev.device)
        s0, r0 = search_masked(L, dev, q, 10, n, m, mode="scan")
        s1, r1 = search_masked(L, dev, q, 10, n, m, mode="mfma")
        assert same_bits(s0, s1) and np.array_equal(r0, r1), name
        assert np.all(flags[r1])
        fallbacks = dev.gemm_timing_read()[3]
        if name == "tail":
            assert fallbacks > 0, "the masked fallback scan did not run"
    Xs = dev.stored_rows(n).cpu().numpy()
    _check_vs_oracle(Xs, Q, tail, 10, s1, r1)
    # the int8 filter copy
    dev.set_filter("i8")
    m = dev_mask(pack(half), dev.device)
    s0, r0 = search_masked(L, dev, q, 10, n, m, mode="scan")
    s1, r1 = search_masked(L, dev, q, 10, n, m, mode="mfma")
    assert same_bits(s0, s1) and np.array_equal(r0, r1)
    _check_vs_oracle(Xs, Q, half, 10, s1, r1)
    # auto with a mask scans (and equals both)
    s2, r2 = search_masked(L, dev, q, 10, n, m, mode="auto")
    assert same_bits(s0, s2) and np.array_equal(r0, r2)
    dev.close()


# ------------------------------------------------------------------- sharded --
@pytest.mark.parametrize("remote", [False, True])
def test_sharded_masked_search_equals_one_index(idxmod, L, cuda, remote):
    import torch

    lib = L.load()
    n, dim = 1003, 96
    X, Q = data(n, dim, 4, 61)
    ss = idxmod.ShardSet(dim, dtype="float16", capacity_per_shard=512, devices=[0, 0, 0])
    if remote:
        ss.force_remote()
    ss.upsert_rows(torch.from_numpy(X), torch.arange(n))
    one = make_index(idxmod, cuda, X, "float16")
    q = torch.from_numpy(Q)
    rng = np.random.default_rng(63)
    flags = rng.random(n) < 0.3
    flags[n - 1] = True
    bm = pack(flags)
    for k in (5, 17):
        s_ref, r_ref = search_masked(L, one, q, k, n, dev_mask(bm, one.device))
        s, r = ss.search(q, k, n, mode="scan", mask=bm)
        torch.cuda.synchronize()
        assert same_bits(s_ref, s.cpu().numpy()) and np.array_equal(r_ref, r.cpu().numpy()), k
        sc, rw, val = ss.query_host(Q.copy(), k, n, True, mask=bm)
        assert same_bits(s_ref, sc) and np.array_equal(r_ref, rw)
        for qi in range(4):
            for j in range(k):
                assert np.array_equal(val[qi, j], ss.fetch_rows([int(rw[qi, j])])[0].numpy())
    # an empty-handed mask and a mask with fewer eligible rows than k, through both calls
    few = np.zeros(n, bool)
    few[[4, 500, 1002]] = True
    s_ref, r_ref = search_masked(L, one, q, 5, n, dev_mask(pack(few), one.device))
    sc, rw, val = ss.query_host(Q.copy(), 5, n, True, mask=pack(few))
    assert same_bits(s_ref, sc) and np.array_equal(r_ref, rw)
    assert np.all(rw[:, 3:] == -1) and np.isnan(val[:, 3:]).all() and sorted(rw[0, :3].tolist()) == [4, 500, 1002]
    # steady state: the second and third identical calls allocate nothing
    ss.search(q, 17, n, mode="scan", mask=bm)
    ss.query_host(Q.copy(), 17, n, True, mask=bm)
    torch.cuda.synchronize()
    n0 = lib.rc_alloc_count()
    for _ in range(2):
        ss.search(q, 17, n, mode="scan", mask=bm)
        ss.query_host(Q.copy(), 17, n, True, mask=bm)
    torch.cuda.synchronize()
    assert lib.rc_alloc_count() == n0
    one.close()
    ss.close()


# --------------------------------------------------------------- Index level --
def _meta(i):
    return {"album": i % 7, "tag": ["even" if i % 2 == 0 else "odd", f"m{i % 5}"], "ts": i}


@pytest.mark.parametrize("shards", [1, 2])
def test_index_query_with_metadata_filter(idxmod, cuda, shards):
    import torch

    n, dim = 500, 64
    X, Q = data(n, dim, 3, 71)
    ix = idxmod.Index(f"filtered-{shards}", dimension=dim, capacity=1024, device=cuda, shards=shards)
    ix.upsert([(f"v{i}", X[i].tolist(), _meta(i)) for i in range(n)])
    Xs = ix.shard_set.fetch_rows(list(range(n)), stored=True).numpy()
    i_ = np.arange(n)
    cases = [
        ({"album": 3}, i_ % 7 == 3),
        ({"ts": {"$gte": 400}}, i_ >= 400),
        ({"$or": [{"tag": "m2"}, {"ts": {"$lt": 20}}]}, (i_ % 5 == 2) | (i_ < 20)),
        ({"album": 99}, np.zeros(n, bool)),
        ({"album": 3, "tag": "odd", "ts": {"$gt": 480}}, (i_ % 7 == 3) & (i_ % 2 == 1) & (i_ > 480)),  # fewer than top_k
    ]
    k = 10
    for flt, flags in cases:
        batch = ix.query_batch(torch.from_numpy(Q), top_k=k, filter=flt, include_metadata=True)
        for qi in range(3):
            got = ix.query(vector=Q[qi].tolist(), top_k=k, filter=flt, include_values=(qi == 0))["matches"]
            if not flags.any():
                assert got == [] and batch[qi]["matches"] == []
                continue
            ref_r, ref_s = _subset_oracle(Xs, Q[qi:qi + 1], flags, k)
            rows = [int(m["id"][1:]) for m in got]
            assert len(rows) == min(k, int(flags.sum()))
            assert topk_equal_modulo_ties(rows, [m["score"] for m in got], ref_r[0], ref_s[0], 1e-5), (flt, qi)
            assert [m["id"] for m in batch[qi]["matches"]] == [m["id"] for m in got]
            assert all(flags[int(m["id"][1:])] and m["metadata"] == _meta(int(m["id"][1:])) for m in batch[qi]["matches"])
            if qi == 0:
                assert np.allclose(got[0]["values"], X[rows[0]], rtol=1e-5, atol=1e-6)
    # filter=None and filter={} are the unfiltered query
    plain = ix.query(vector=Q[0].tolist(), top_k=k)
    assert ix.query(vector=Q[0].tolist(), top_k=k, filter=None) == plain
    assert ix.query(vector=Q[0].tolist(), top_k=k, filter={}) == plain
    assert ix.query_batch(torch.from_numpy(Q[:1]), top_k=k, filter={})[0]["matches"] == plain["matches"]
    unfiltered_rows = {int(m["id"][1:]) for m in plain["matches"]}
    assert any(r % 7 != 3 for r in unfiltered_rows)  # so {"album": 3} above really restricted something
    # an upsert that changes one vector's metadata invalidates the cached bitmap
    target = 5  # album 5
    flt = {"album": 3}
    before = ix.query(vector=X[target].tolist(), top_k=1, filter=flt)["matches"]
    assert before[0]["id"] != f"v{target}"
    ix.upsert([(f"v{target}", X[target].tolist(), {**_meta(target), "album": 3})])
    after = ix.query(vector=X[target].tolist(), top_k=1, filter=flt)["matches"]
    assert after[0]["id"] == f"v{target}" and abs(after[0]["score"] - 1.0) < 1e-5
    assert len(ix._bitmaps) <= 8
    with pytest.raises(ValueError):
        ix.query(vector=Q[0].tolist(), top_k=k, filter={"album": {"$bogus": 1}})
    with pytest.raises(ValueError):
        ix.query(vector=Q[0].tolist(), top_k=k, filter=["album"])
    ix.close()


def test_query_batch_auto_takes_mfma_for_dense_filters_only(idxmod, cuda):
    """65,536 f16 rows, 8 queries: ``mode="auto"`` runs the filter GEMM for a filter that keeps 3
    rows of 4 (share 0.75 >= MASKED_MFMA_MIN_SHARE) and the masked scan for one that keeps 1 of
    4; both equal the forced masked scan."""
    import torch

    assert 0.25 < idxmod.MASKED_MFMA_MIN_SHARE <= 0.75
    n, dim = 65536, 128
    X, Q = data(n, dim, 8, 81)
    ix = idxmod.Index("filtered-auto", dimension=dim, dtype="float16", capacity=n, device=cuda)
    ids = [f"v{i}" for i in range(n)]
    ix.upsert_tensor(ids, torch.from_numpy(X).to(cuda), [{"g": i % 4} for i in range(n)])
    dev = ix.shard_set.shard(0)
    dev.timing(True)
    q = torch.from_numpy(Q)
    for flt, want_gemm in (({"g": {"$ne": 3}}, True), ({"g": 3}, False)):
        ref = ix.query_batch(q, top_k=10, filter=flt, mode="scan")
        dev.gemm_timing_read()
        got = ix.query_batch(q, top_k=10, filter=flt)
        launches = dev.gemm_timing_read()[1]
        assert got == ref
        assert (launches > 0) == want_gemm, (flt, launches)
        keep = (lambda g: g != 3) if want_gemm else (lambda g: g == 3)
        assert all(len(r["matches"]) == 10 and all(keep(int(m["id"][1:]) % 4) for m in r["matches"]) for r in got)
    ix.close()
