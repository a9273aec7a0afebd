"""GPU tests of the streaming int8 filter (RC_FILTER_I8_STREAM): its kernel's keep-test value against
float64, and ``mode="mfma"`` with 1 to 8 queries against ``mode="scan"``, BIT FOR BIT (rows and scores)."""
import numpy as np
import pytest
import torch

from conftest import import_pkg

pytestmark = pytest.mark.gpu

CAP = 4096  # BATCH_CAND_CAP: the first stage's rows and a query's candidate slots per stage
DIMS = [200, 512, 768]  # row widths 256, 512, 768


def stage_ratio(k):  # batch_stage_ratio(k, CAP, I8_STAGE_INFLATION = 3)
    return max(2, min(64, CAP // (5 * k // 2 * 3 + 1)))


N_MAX = CAP * stage_ratio(1) + 77
_DEVS = {}


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


@pytest.fixture(scope="module")
def devs(idxmod, cuda):
    """(DeviceIndex with the "i8_stream" filter, 8 queries) per (dim, dtype): N_MAX Gaussian rows, left unchanged."""
    def get(dim, dtype):
        if (dim, dtype) not in _DEVS:
            g = torch.Generator(device=cuda).manual_seed(1907 + dim)
            dev = idxmod.DeviceIndex(dim, dtype=dtype, capacity=N_MAX, device=cuda)
            dev.upsert_rows(torch.randn((N_MAX, dim), generator=g, device=cuda), torch.arange(N_MAX))
            dev.set_filter("i8_stream")
            _DEVS[dim, dtype] = (dev, torch.randn((8, dim), generator=g, device=cuda).cpu())
        return _DEVS[dim, dtype]

    yield get
    for dev, _ in _DEVS.values():
        dev.close()
    _DEVS.clear()


def assert_mfma_equals_scan(dev, Q, k, n, mask=None):
    s, r = dev.search(Q, k, n, mode="mfma", mask=mask)
    s2, r2 = dev.search(Q, k, n, mode="scan", mask=mask)
    assert torch.equal(r, r2) and torch.equal(s.view(torch.int32), s2.view(torch.int32)), (k, n)


def quantise(v):  # the documented rule, in float64: each vector's residual norm ||v - sx·v8||
    sx = np.abs(v).max(axis=1, keepdims=True) / 127.0
    v8 = np.clip(np.rint(np.divide(v, sx, out=np.zeros_like(v), where=sx > 0)), -127, 127)
    return np.linalg.norm(v - sx * v8, axis=1)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("dim", DIMS)
def test_kernel_against_float64(idxmod, cuda, dim, dtype):
    row0, n = 128, 1000
    rng = np.random.Generator(np.random.PCG64(11 + dim))
    X = rng.standard_normal((row0 + n, dim)).astype(np.float32)
    Q = rng.standard_normal((8, dim)).astype(np.float32)
    X[row0 + 5] = 3.0 * Q[0]  # a row equal to a query,
    X[row0 + 6] = 0.0
    X[row0 + 6, dim // 2] = 2.0  # one all in one component,
    X[row0 + 999] = 0.0
    X[row0 + 999, dim - 1] = 1e-12  # and one whose single non-zero component is tiny
    dev = idxmod.DeviceIndex(dim, dtype=dtype, capacity=row0 + n, device=cuda)
    dev.upsert_rows(torch.from_numpy(X), torch.arange(row0 + n))
    dev.set_filter("i8_stream")
    xh = dev.stored_rows(row0 + n).cpu().numpy().astype(np.float64)[row0:]
    qh = Q.astype(np.float64) / np.linalg.norm(Q.astype(np.float64), axis=1, keepdims=True)
    ex, eq = quantise(xh), quantise(qh)
    for nq in (1, 3, 8):
        u, eps = (t.cpu().numpy().astype(np.float64) for t in dev.filter_scores(torch.from_numpy(Q[:nq]), row0, n))
        c = qh[:nq] @ xh.T
        # the issue's 2·ex·aq + 1.01·eq + 1e-5: aq is the kernel's own 1.0001 + eq
        slack = 2.0 * ex[None, :] * (1.0001 + eq[:nq, None]) + 1.01 * eq[:nq, None] + 1e-5
        assert np.all(u + eps[:, None] >= c)  # the filter can never drop a member
        assert np.all(u - c <= slack)  # and it is a bound, not +inf
    dev.close()


@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("k", [1, 10, 256])
@pytest.mark.parametrize("nq", [1, 3, 8])
def test_search_equals_scan(devs, dim, dtype, k, nq):
    dev, Q = devs(dim, dtype)
    for n in (3000, CAP * stage_ratio(k) + 77):  # one stage; three stages and a ragged last tile
        assert_mfma_equals_scan(dev, Q[:nq], k, n)
    s, r = dev.search(Q[:nq], k, 0, mode="mfma")  # an empty index
    assert (r == -1).all() and (s == -float("inf")).all()


def test_overflow_falls_back_on_the_device(idxmod, cuda):
    n, dim = 20_000, 512
    X = np.random.Generator(np.random.PCG64(3)).standard_normal((n, dim)).astype(np.float32)
    X[5000:11000] = X[17]  # 6,000 copies past the first stage: more than a stage's CAP slots
    dev = idxmod.DeviceIndex(dim, dtype="float16", capacity=n, device=cuda)
    dev.upsert_rows(torch.from_numpy(X), torch.arange(n))
    dev.set_filter("i8_stream")
    dev.timing(True)
    dev.gemm_timing_read()
    assert_mfma_equals_scan(dev, torch.from_numpy(X[17:18]), 10, n)
    assert dev.gemm_timing_read()[3] >= 1
    dev.close()


def test_mask_is_applied_by_the_rescoring(devs, cuda):
    dev, Q = devs(512, "float16")
    n = CAP * stage_ratio(10) + 77
    eligible = np.random.Generator(np.random.PCG64(23)).random(n) < 0.05
    words = np.packbits(np.pad(eligible, (0, -n % 32)), bitorder="little").view(np.int32)
    assert_mfma_equals_scan(dev, Q[:1], 10, n, mask=torch.from_numpy(words.copy()).to(cuda))


def test_copy_follows_writes_and_the_two_int8_kinds_share_it(idxmod, cuda):
    n, dim = 6000, 200  # past the first stage's CAP rows, where the filter reads the copy
    g = torch.Generator().manual_seed(5)
    dev = idxmod.DeviceIndex(dim, dtype="float16", capacity=n, device=cuda)
    dev.upsert_rows(torch.randn((n, dim), generator=g), torch.arange(n))
    dev.set_filter("i8_stream")
    Q = torch.randn((3, dim), generator=g)
    dev.upsert_rows(torch.randn((500, dim), generator=g), torch.arange(4500, 5000))
    dev.upsert_rows(3.0 * Q[1:2], torch.tensor([100]))
    dev.move_rows(torch.tensor([100]), torch.tensor([5500]))  # the best row of query 1, moved
    dev.grow(2 * n)
    dev.upsert_rows(2.0 * Q[:1], torch.tensor([n + 200]))  # the best row of query 0, in the grown part
    assert_mfma_equals_scan(dev, Q, 10, n + 300)
    top = dev.search(Q, 10, n + 300, mode="mfma")[1]
    assert top[0, 0] == n + 200 and sorted(top[1, :2].tolist()) == [100, 5500]
    count = dev.lib.rc_alloc_count()
    assert_mfma_equals_scan(dev, Q, 10, n + 300)  # a repeated search allocates nothing,
    for kind in ("i8", "i8_stream", "i8"):  # and the two int8 kinds share the copy
        dev.set_filter(kind)
        assert dev.filter == kind
    assert dev.lib.rc_alloc_count() == count
    dev.close()


def test_through_the_public_path(idxmod, cuda, tmp_path):
    """The constructor, the sharded set_filter and save / load.  At this size ``auto`` is on the scan under
    both kinds, so the answers compared are the scan's: the new kernel is reached by the tests above."""
    n, dim = 5000, 512
    g = torch.Generator().manual_seed(9)
    X, Q = torch.randn((n, dim), generator=g), torch.randn((3, dim), generator=g)
    res = {}
    for kind in ("native", "i8_stream"):
        idx = idxmod.Index("s", dimension=dim, dtype="float32", capacity=n, device=cuda, shards=2, filter=kind)
        idx.upsert_tensor([f"v{i}" for i in range(n)], X.to(cuda))
        res[kind] = (idx.query(Q[0].tolist(), top_k=5)["matches"], idx.query_batch(Q, top_k=5))
        if kind == "i8_stream":
            idx.save(str(tmp_path))
            back = idxmod.Index.load(str(tmp_path), device=cuda)
            assert back.shard_set.filter == "i8_stream"
            back.close()
        idx.close()
    assert res["i8_stream"] == res["native"]


def test_nine_queries_run_the_int8_filter(devs, cuda):
    dev, Q = devs(512, "float16")
    Q9 = torch.cat([Q, Q[:1] + Q[1:2]])
    n = CAP * stage_ratio(10) + 77
    got = dev.search(Q9, 10, n, mode="mfma")
    dev.set_filter("i8")
    try:
        want = dev.search(Q9, 10, n, mode="mfma")
    finally:
        dev.set_filter("i8_stream")
    assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
