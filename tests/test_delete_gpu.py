"""GPU tests of ``Index.delete``: the row-move kernel (``rc_index_move_rows``), its sharded form
(``rc_sharded_move_rows``: inside a shard, between shards, and through the pack / peer copy /
unpack path that ``force_remote`` drives on one GPU), the host maps, and the ``/delete_images``
route.

Every comparison is bit for bit.  The reference for a deleted-from index is a fresh ``Index``
upserted with the survivors' original f32 vectors in the row order ``plan_compaction`` predicts:
an upsert normalises each vector on its own, so equal vectors give equal stored bits whatever
their row, and equal stored rows in equal order give equal scores and equal tie order.  Rows at
or past the new length keep stale bytes (the fresh index has zeros there); the searches must
never score them.
"""
import io
import os

import numpy as np
import pytest
from fastapi.testclient import TestClient

from conftest import GOLDEN, import_pkg

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float16", "bfloat16"]
N = 1000


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


@pytest.fixture(scope="module")
def plan():
    return import_pkg("compaction").plan_compaction


_DATA = {}


def data(dim):
    """Rows and queries, computed once per width and left unchanged."""
    if dim not in _DATA:
        rng = np.random.default_rng(4000 + dim)
        _DATA[dim] = (rng.standard_normal((N, dim)).astype(np.float32), rng.standard_normal((9, dim)).astype(np.float32))
    return _DATA[dim]


# 37 tail rows into 37 scattered holes: holes 127 / 128 straddle a 128-row tile edge, the sources
# lie on both sides of row 896 (the last tile edge below N)
HOLES = [0, 1, 5, 31, 32, 63, 64, 100, 127, 128, 129, 200, 255, 256, 257, 300, 333, 383, 384, 400, 450, 499, 500, 511,
         512, 513, 600, 640, 700, 767, 768, 769, 800, 850, 860, 870, 880]
SOURCES = [999, 890, 895, 896, 897, 900, 998, 891, 950, 901, 892, 960, 893, 902, 970, 894, 903, 980, 904, 990, 905, 991,
           906, 992, 907, 993, 908, 994, 909, 995, 910, 996, 911, 997, 912, 913, 889]
assert len(HOLES) == len(SOURCES) == 37 and not set(HOLES) & set(SOURCES)
assert len(set(HOLES)) == 37 and len(set(SOURCES)) == 37


def export(dev, n=N):
    import torch

    rows, norms = dev.export_rows(0, n)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), norms.cpu().numpy()


def make_dev(idxmod, cuda, X, dtype, capacity=N):
    import torch

    dev = idxmod.DeviceIndex(X.shape[1], dtype=dtype, capacity=capacity, device=cuda)
    dev.upsert_rows(torch.from_numpy(X), torch.arange(X.shape[0], dtype=torch.int64))
    return dev


# ---------------------------------------------------------------- kernel level --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [128, 768, 1000])  # dim 1000: ld = 1024 > dim (the stored width is what moves)
def test_move_rows_copies_bits_and_norms(idxmod, cuda, dtype, dim):
    import torch

    X, _ = data(dim)
    X = X * np.linspace(0.5, 3.0, N, dtype=np.float32)[:, None]  # distinct norms: a norm left behind shows
    dev = make_dev(idxmod, cuda, X, dtype)
    rows0, norms0 = export(dev)
    assert rows0.shape[1] == dev.ld * (4 if dtype == "float32" else 2) and dev.ld == (dim + 127) // 128 * 128
    dev.move_rows(SOURCES, HOLES)
    rows1, norms1 = export(dev)
    want_r, want_n = rows0.copy(), norms0.copy()
    want_r[HOLES] = rows0[SOURCES]
    want_n[HOLES] = norms0[SOURCES]
    # the holes hold the sources' bytes and norms; every other row, the now-stale tail included, is unchanged
    assert np.array_equal(rows1, want_r)
    assert np.array_equal(norms1.view(np.uint32), want_n.view(np.uint32))
    # an index outside [0, capacity) in either list skips its pair: nothing is read or written
    cap = dev.capacity
    dev.move_rows([cap, 3, -1, cap + 7, 1 << 40], [10, cap, 11, -5, 12])
    rows2, norms2 = export(dev)
    assert np.array_equal(rows2, want_r) and np.array_equal(norms2.view(np.uint32), want_n.view(np.uint32))
    with pytest.raises(ValueError):
        dev.move_rows([1, 2], [3])
    dev.move_rows(torch.empty(0, dtype=torch.int64), [])  # nothing to do
    dev.close()


def test_move_rows_refreshes_the_int8_copy(idxmod, cuda):
    """f16, 512 wide, int8 filter: after the move the MFMA search (int8 filter GEMM, exact rescoring)
    returns exactly the scan's lists and names the destination row first for a query built from
    the moved row.  A stale int8 row at the destination would bound the true row's score from
    the old row's values and drop it."""
    import torch

    X, _ = data(512)
    dev = make_dev(idxmod, cuda, X, "float16")
    dev.set_filter("i8")
    dev.move_rows(SOURCES, HOLES)
    rng = np.random.default_rng(7)
    q = X[SOURCES] + 0.05 * rng.standard_normal((len(SOURCES), 512)).astype(np.float32)
    n_live = min(SOURCES)  # the rows a delete would leave: every hole is below, every source at or above
    assert max(HOLES) < n_live
    ss, rs = dev.search(torch.from_numpy(q), 10, n_live, mode="scan")
    sm, rm = dev.search(torch.from_numpy(q), 10, n_live, mode="mfma")
    torch.cuda.synchronize()
    assert np.array_equal(rs.cpu().numpy(), rm.cpu().numpy())
    assert np.array_equal(ss.cpu().numpy().view(np.uint32), sm.cpu().numpy().view(np.uint32))
    assert rm.cpu().numpy()[:, 0].tolist() == HOLES
    dev.close()


# ------------------------------------------------- Index.delete vs a rebuilt index --
def ids_of(order):
    return [f"v{i}" for i in order]


def build_index(idxmod, cuda, X, order, dtype, shards, remote=False, name="delete-test"):
    import torch

    # f32 takes the int8 filter so that mode="mfma" exists for it too (and delete keeps that copy right)
    idx = idxmod.Index(name, dimension=X.shape[1], dtype=dtype, capacity=N, device=cuda, shards=shards,
                       filter="i8" if dtype == "float32" else "native")
    if remote:
        idx.shard_set.force_remote()
    if order:
        idx.upsert_tensor(ids_of(order), torch.from_numpy(X[order]).to(cuda), [{"label": i % 7} for i in order])
    return idx


def same_matches(a, b):
    assert [m["id"] for m in a] == [m["id"] for m in b]
    assert np.array_equal(np.asarray([m["score"] for m in a], np.float32).view(np.uint32),
                          np.asarray([m["score"] for m in b], np.float32).view(np.uint32))
    for ma, mb in zip(a, b):
        assert ("values" in ma) == ("values" in mb)
        if "values" in ma:
            assert ma["values"] == mb["values"]


def compare_with_rebuilt(idx, ref, Q):
    assert len(idx) == len(ref)
    for q in Q[:2]:
        for values in (False, True):
            same_matches(idx.query(vector=q.tolist(), top_k=10, include_values=values)["matches"],
                         ref.query(vector=q.tolist(), top_k=10, include_values=values)["matches"])
        same_matches(idx.query(vector=q.tolist(), top_k=10, filter={"label": {"$in": [1, 2]}})["matches"],
                     ref.query(vector=q.tolist(), top_k=10, filter={"label": {"$in": [1, 2]}})["matches"])
    import torch

    for mode in ("scan", "mfma"):
        got = idx.query_batch(torch.from_numpy(Q), top_k=10, mode=mode)
        want = ref.query_batch(torch.from_numpy(Q), top_k=10, mode=mode)
        for g, w in zip(got, want):
            same_matches(g["matches"], w["matches"])


# one shard; three shards through pack / peer copy / unpack (force_remote); three shards of one
# GPU as a default Index(shards=3) runs them: cross-shard pairs in one launch from shard to shard
SHARDINGS = [pytest.param(1, False, id="1"), pytest.param(3, True, id="3-remote"), pytest.param(3, False, id="3-direct")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shards,remote", SHARDINGS)
def test_delete_equals_a_rebuilt_index(idxmod, plan, cuda, dtype, shards, remote):
    X, Q = data(256)
    order = list(range(N))
    idx = build_index(idxmod, cuda, X, order, dtype, shards, remote=remote)
    rows0, norms0 = idx.shard_set.export_rows(N)
    rng = np.random.default_rng(99)

    def patterns():
        yield "one middle id", [order[len(order) // 2]], []
        yield "the last id only", [order[-1]], []
        yield "the whole tail", order[-60:], []
        yield "a random 30 %", [order[i] for i in rng.choice(len(order), int(0.3 * len(order)), replace=False)], []
        some = [order[3], order[40], order[200]]
        yield "unknown and repeated ids", some, ["nope", ids_of(some)[0], "v-1", ids_of(some)[2], ""]
        yield "all but one", [i for i in order if i != order[17]], []
        yield "everything", list(order), []

    for what, dead, extra in patterns():
        rows = sorted(order.index(i) for i in dead)
        src, dst = plan(len(order), rows, shards)
        for s, d in zip(src, dst):
            order[d] = order[s]
        del order[len(order) - len(rows):]
        assert idx.delete(ids=ids_of(dead) + extra) == {}
        assert len(idx) == len(order) and idx._ids == ids_of(order), what
        assert idx.describe_index_stats()["total_vector_count"] == len(order)
        got_r, got_n = idx.shard_set.export_rows(len(idx))
        assert np.array_equal(got_r, rows0[order]), what
        assert np.array_equal(got_n.view(np.uint32), norms0[order].view(np.uint32)), what
        if not order:
            assert idx.query(vector=Q[0].tolist(), top_k=10)["matches"] == []
            assert idx.query_batch(Q.tolist(), top_k=10)[0]["matches"] == []
            continue
        ref = build_index(idxmod, cuda, X, order, dtype, shards, name="rebuilt")
        compare_with_rebuilt(idx, ref, Q)
        ref.close()
    assert len(idx) == 0 and idx.capacity >= N  # capacity never shrinks
    idx.close()


# --------------------------------------------------------- state after a delete --
@pytest.fixture(params=[True, False], ids=["remote", "direct"])
def small(request, idxmod, cuda):
    X, Q = data(128)
    idx = build_index(idxmod, cuda, X, list(range(N)), "float16", 3, remote=request.param)
    yield idx, X, Q
    idx.close()


def test_fetch_and_cached_values_after_delete(small):
    idx, X, Q = small
    before = idx.fetch(ids_of(range(N - 5, N)))["vectors"]
    m = idx.query(vector=X[N - 1].tolist(), top_k=5, include_values=True)["matches"]
    assert m[0]["id"] == f"v{N - 1}"
    hit_ids = [x["id"] for x in m]
    idx.delete(ids=["v3", "v4", hit_ids[1]])
    assert idx._recent[0] != idx._gen  # the values that query cached cannot serve the next fetch
    got = idx.fetch(["v3", "v4"] + hit_ids + ids_of(range(N - 5, N)))["vectors"]
    assert "v3" not in got and "v4" not in got and hit_ids[1] not in got
    # moved ids (the tail filled the holes) return their own values, bit for bit
    moved = [i for i in ids_of(range(N - 5, N)) if i in got]
    assert len(moved) >= 4 and any(idx._rows[i] in (3, 4) for i in moved)
    for i in moved:
        assert got[i]["values"] == before[i]["values"] and got[i]["metadata"] == before[i]["metadata"]
    assert idx.fetch([hit_ids[0]])["vectors"][hit_ids[0]]["values"] == m[0]["values"]


def test_filter_bitmap_is_rebuilt_after_delete(small, idxmod, cuda):
    idx, X, Q = small
    flt = {"label": {"$in": [1, 2]}}
    q = Q[0].tolist()
    first = idx.query(vector=q, top_k=10, filter=flt)["matches"]
    dead = [x["id"] for x in first[:3]] + ["v0", "v1", "v2", "v8", "v9"]
    idx.delete(ids=dead)
    order = [int(i[1:]) for i in idx._ids]
    ref = build_index(idxmod, cuda, X, order, "float16", 3, name="rebuilt")
    same_matches(idx.query(vector=q, top_k=10, filter=flt)["matches"], ref.query(vector=q, top_k=10, filter=flt)["matches"])
    again = idx.query(vector=q, top_k=10, filter=flt, include_metadata=True)["matches"]
    assert not {x["id"] for x in again} & set(dead) and all(x["metadata"]["label"] in (1, 2) for x in again)
    ref.close()


def test_upsert_after_delete_reuses_the_freed_rows(small):
    idx, X, Q = small
    cap = idx.capacity
    idx.delete(ids=ids_of(range(100, 140)))
    assert len(idx) == N - 40
    rng = np.random.default_rng(3)
    new = rng.standard_normal((40, X.shape[1])).astype(np.float32)
    idx.upsert([(f"new{i}", new[i].tolist(), {"label": 100}) for i in range(40)])
    assert len(idx) == N and idx.capacity == cap
    assert sorted(idx._rows[f"new{i}"] for i in range(40)) == list(range(N - 40, N))
    stats = idx.describe_index_stats()
    assert stats["total_vector_count"] == N and stats["namespaces"][""]["vector_count"] == N
    for i in (0, 17, 39):
        assert idx.query(vector=new[i].tolist(), top_k=1)["matches"][0]["id"] == f"new{i}"
    import torch

    res = idx.query_batch(torch.from_numpy(new[:9]), top_k=1, mode="mfma")
    assert [r["matches"][0]["id"] for r in res] == [f"new{i}" for i in range(9)]


def test_save_load_round_trips_a_compacted_index(small, idxmod, cuda, tmp_path):
    idx, X, Q = small
    idx.delete(ids=ids_of(range(0, N, 3)))
    idx.save(str(tmp_path / "snap"))
    back = idxmod.Index.load(str(tmp_path / "snap"), device=cuda)
    assert back._ids == idx._ids and len(back) == len(idx)
    r0, n0 = idx.shard_set.export_rows(len(idx))
    r1, n1 = back.shard_set.export_rows(len(back))
    assert np.array_equal(r0, r1) and np.array_equal(n0.view(np.uint32), n1.view(np.uint32))
    for q in Q[:2]:
        same_matches(idx.query(vector=q.tolist(), top_k=10, include_values=True, filter={"label": 3})["matches"],
                     back.query(vector=q.tolist(), top_k=10, include_values=True, filter={"label": 3})["matches"])
    back.close()


def test_delete_by_filter_and_by_everything(small):
    idx, X, Q = small
    assert idx.delete(filter={"label": {"$in": [0, 6]}}) == {}
    want = [i for i in range(N) if i % 7 not in (0, 6)]
    assert sorted(int(i[1:]) for i in idx._ids) == want and len(idx) == len(want)
    assert set(idx.fetch(ids_of(range(N)))["vectors"]) == set(ids_of(want))
    assert idx.delete(filter={"label": 99}) == {} and len(idx) == len(want)  # nothing matches: nothing happens
    assert idx.delete(ids=[]) == {} and len(idx) == len(want)
    assert idx._delete(["v1", "v1", "v7", "nope"], False, None) == 1  # the route's count; v7 (label 0) is already gone
    assert idx.delete(delete_all=True) == {}
    assert len(idx) == 0 and idx.query(vector=Q[0].tolist(), top_k=3)["matches"] == []
    assert idx.fetch(["v2"])["vectors"] == {}
    idx.upsert([("again", X[0].tolist(), {})])
    assert idx.query(vector=X[0].tolist(), top_k=3)["matches"][0]["id"] == "again" and len(idx) == 1


def test_delete_needs_exactly_one_selector(small):
    idx, X, Q = small
    for kw in ({}, {"filter": {}}, {"ids": ["v1"], "filter": {"label": 1}}, {"ids": ["v1"], "delete_all": True},
               {"delete_all": True, "filter": {"label": 1}}, {"ids": "v1"}, {"filter": "label"}):
        with pytest.raises(ValueError):
            idx.delete(**kw)
    assert len(idx) == N


def test_failed_device_move_removes_no_id_and_can_be_repeated(small, idxmod, cuda, monkeypatch):
    """The contract in delete's docstring, without any fault: the device call is made to raise."""
    idx, X, Q = small
    ids0, rows0, meta0, gen0 = list(idx._ids), dict(idx._rows), {k: dict(v) for k, v in idx._meta.items()}, idx._gen
    dead = ids_of([2, 3, 500, N - 2])
    calls = []

    def boom(src, dst):
        calls.append((list(src), list(dst)))
        raise RuntimeError("device move failed")

    monkeypatch.setattr(idx.shard_set, "move_rows", boom)
    with pytest.raises(RuntimeError, match="device move failed"):
        idx.delete(ids=dead)
    assert len(calls) == 1 and calls[0][1] == [2, 3, 500]  # the holes; row N - 2 is in the tail
    assert idx._ids == ids0 and idx._rows == rows0 and idx._meta == meta0 and len(idx) == N
    assert idx._gen > gen0  # nothing cached before the call can be served after it
    assert set(idx.fetch(dead)["vectors"]) == set(dead)
    monkeypatch.undo()
    assert idx.delete(ids=dead) == {} and len(idx) == N - 4
    order = [int(i[1:]) for i in idx._ids]
    assert sorted(order) == sorted(set(range(N)) - {2, 3, 500, N - 2})
    ref = build_index(idxmod, cuda, X, order, "float16", 3, name="rebuilt")
    for q in Q[:2]:
        same_matches(idx.query(vector=q.tolist(), top_k=10, include_values=True)["matches"],
                     ref.query(vector=q.tolist(), top_k=10, include_values=True)["matches"])
    ref.close()


@pytest.mark.parametrize("remote", [True, False], ids=["remote", "direct"])
def test_sharded_move_rows_in_several_rounds(idxmod, cuda, remote):
    """More pairs than one round of rc_sharded_move_rows holds (16384), after a small call that
    sized the staging: the rounds, and the staging regrown between calls, byte for byte.  40 000
    synthetic rows of 128 f16 (10 MB); the last 20 000 rows move into the first 20 000 in a random
    order, so that about two pairs in three cross shards."""
    n, half = 40_000, 20_000
    ss = idxmod.ShardSet(128, dtype="float16", capacity_per_shard=(n + 2) // 3, devices=[cuda] * 3)
    if remote:
        ss.force_remote()
    for s in range(3):
        ss.shard(s).fill_random(5 + s, 0, ss.shard_rows(s, n))
    rows0, norms0 = ss.export_rows(n)
    assert len(np.unique(norms0)) > n // 2  # the norms tell rows apart too
    want_r, want_n = rows0.copy(), norms0.copy()
    ss.move_rows([n - 1, n - 2, n - 3], [1, 5, 6])  # sizes the staging for 3 rows
    want_r[[1, 5, 6]], want_n[[1, 5, 6]] = rows0[[n - 1, n - 2, n - 3]], norms0[[n - 1, n - 2, n - 3]]
    src = np.arange(half, n)
    dst = np.random.default_rng(21).permutation(half)
    ss.move_rows(src, dst)
    want_r[dst], want_n[dst] = rows0[src], norms0[src]
    got_r, got_n = ss.export_rows(n)
    assert np.array_equal(got_r, want_r) and np.array_equal(got_n.view(np.uint32), want_n.view(np.uint32))
    ss.close()


def test_sharded_move_rows_validates_before_moving(small):
    idx, X, Q = small
    ss = idx.shard_set
    rows0, norms0 = ss.export_rows(N)
    cap = ss.capacity
    for src, dst in (([5, 5], [1, 2]), ([5, 6], [1, 1]), ([5, 6], [6, 1]), ([5, cap], [1, 2]), ([5, 6], [1, -1])):
        with pytest.raises(ValueError):
            ss.move_rows(src, dst)
    rows1, norms1 = ss.export_rows(N)
    assert np.array_equal(rows0, rows1) and np.array_equal(norms0.view(np.uint32), norms1.view(np.uint32))


# ------------------------------------------------------------------------ route --
def _jpeg(seed, w=224, h=224):
    from PIL import Image

    arr = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="JPEG", quality=85)
    return b.getvalue()


def test_delete_images_route(cuda, monkeypatch):
    cfg = import_pkg("config").Config
    monkeypatch.setattr(cfg, "INDEX_NAME", "delete-images-route")
    svc = TestClient(import_pkg("service").app)
    with open(os.path.join(GOLDEN, "test_image.jpeg"), "rb") as f:
        fixture = f.read()
    first = svc.post("/push_image", files={"file": ("fixture.jpeg", fixture, "image/jpeg")}).json()
    others = [("files", (f"o{i}.jpg", _jpeg(300 + i), "image/jpeg")) for i in range(6)]
    batch = svc.post("/push_images", files=others).json()
    ix = import_pkg("service").index()
    assert len(ix) == 7
    assert svc.post("/search_image", files={"file": ("q.jpeg", fixture, "image/jpeg")}).json()[0] == first["signed_url"]
    for bad in ({"json": {}}, {"json": {"ids": "abc"}}, {"json": {"ids": [1, 2]}}, {"json": [first["file_id"]]},
                {"content": b"not json"}, {}):
        assert svc.post("/delete_images", **bad).status_code == 422
    assert len(ix) == 7
    r = svc.post("/delete_images", json={"ids": [first["file_id"], "no-such-id", batch[2]["file_id"], first["file_id"]]})
    assert r.status_code == 200 and r.json() == {"deleted_count": 2}
    assert len(ix) == 5
    urls = svc.post("/search_image", files={"file": ("q.jpeg", fixture, "image/jpeg")}).json()
    assert len(urls) == 5 and first["signed_url"] not in urls and batch[2]["signed_url"] not in urls
    assert svc.post("/search_image", files={"file": others[4][1]}).json()[0] == batch[4]["signed_url"]
    assert svc.post("/delete_images", json={"ids": []}).json() == {"deleted_count": 0}
    ix.close()
    import_pkg("ingesting.utils")._indexes.pop("delete-images-route", None)
