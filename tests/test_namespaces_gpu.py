"""``Index`` namespaces on the GPU: ``namespace=`` on upsert / query / query_batch / fetch / delete
names an independent vector set (ids are unique per namespace), the default namespace ``""`` is
what it was, and the named ones share a paged pool that is searched through page tables."""
import io
import json
import os

import numpy as np
import pytest

from conftest import import_pkg

pytestmark = pytest.mark.gpu

DIM = 64


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


_DATA = {}


def vectors(n, seed, dim=DIM):
    key = (n, seed, dim)
    if key not in _DATA:
        _DATA[key] = np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)
    return _DATA[key]


def ids_of(n, prefix="v"):
    return [f"{prefix}{i}" for i in range(n)]


def fill(ix, ns, X, ids=None, meta=None, step=700):
    import torch

    ids = ids or ids_of(len(X))
    for i in range(0, len(X), step):
        ix.upsert_tensor(ids[i:i + step], torch.from_numpy(X[i:i + step]).cuda(), None if meta is None else meta[i:i + step],
                         namespace=ns)


def matches(res):
    return [(m["id"], np.float32(m["score"]).view(np.uint32).item()) for m in res["matches"]]


def ranking64(X, q, metric="cosine"):
    """ids' order and float64 scores of the stored directions times their norms (what fetch returns)."""
    X = X.astype(np.float64)
    q = np.asarray(q, np.float64)
    if metric == "cosine":
        s = (X @ q) / (np.linalg.norm(X, axis=1) * np.linalg.norm(q))
        order = np.argsort(-s, kind="stable")
    else:
        s = ((X - q[None]) ** 2).sum(1)
        order = np.argsort(s, kind="stable")
    return order, s


# ------------------------------------------------------------------ isolation --
def test_namespaces_are_isolated_and_the_default_one_is_unchanged(idxmod, cuda):
    A, B, D = vectors(300, 1), vectors(300, 2), vectors(50, 3)
    ix = idxmod.Index("iso", dimension=DIM, capacity=256, device=cuda)
    plain = idxmod.Index("iso-plain", dimension=DIM, capacity=256, device=cuda)
    fill(ix, "", D)
    fill(plain, "", D)
    fill(ix, "a", A)
    fill(ix, "b", B)  # the same ids v0 .. v299, other vectors; v0 .. v49 are in "" too
    assert len(ix) == 50
    q = A[7].tolist()
    ra = ix.query(vector=q, top_k=5, namespace="a", include_values=True)
    assert ra["namespace"] == "a" and ra["matches"][0]["id"] == "v7" and abs(ra["matches"][0]["score"] - 1.0) < 1e-6
    oa, _ = ranking64(A, q)
    assert [m["id"] for m in ra["matches"]] == [f"v{i}" for i in oa[:5]]
    # the values query("a") just returned must not be served to a fetch in "b" or ""
    got = ix.fetch([m["id"] for m in ra["matches"]], namespace="b")
    for vid, rec in got["vectors"].items():
        np.testing.assert_allclose(rec["values"], B[int(vid[1:])], rtol=0, atol=1e-5)
    assert got["namespace"] == "b"
    np.testing.assert_allclose(ix.fetch(["v7"], namespace="a")["vectors"]["v7"]["values"], A[7], rtol=0, atol=1e-5)
    np.testing.assert_allclose(ix.fetch(["v7"])["vectors"]["v7"]["values"], D[7], rtol=0, atol=1e-5)
    rb = ix.query(vector=q, top_k=5, namespace="b")
    ob, sb = ranking64(B, q)
    assert [m["id"] for m in rb["matches"]] == [f"v{i}" for i in ob[:5]] and rb["matches"][0]["score"] < 0.9
    assert ix.fetch(["v299"])["vectors"] == {} and ix.fetch(["v299"], namespace="a")["vectors"]["v299"]["id"] == "v299"
    # "" answers what an index without namespaces answers, bit for bit, on every path
    for kw in ({}, {"filter": None}, {"namespace": None}):
        assert matches(ix.query(vector=q, top_k=10, **kw)) == matches(plain.query(vector=q, top_k=10))
    assert [matches(r) for r in ix.query_batch(D[:9], top_k=7)] == [matches(r) for r in plain.query_batch(D[:9], top_k=7)]
    st = ix.describe_index_stats()
    assert st["namespaces"] == {"": {"vector_count": 50}, "a": {"vector_count": 300}, "b": {"vector_count": 300}}
    assert st["total_vector_count"] == 650
    assert plain.describe_index_stats()["namespaces"] == {"": {"vector_count": 50}}
    for bad in (3, b"a", ["a"]):
        with pytest.raises(ValueError):
            ix.query(vector=q, top_k=5, namespace=bad)
        with pytest.raises(ValueError):
            ix.upsert([("x", q)], namespace=bad)
    ix.close()
    plain.close()


# ----------------------------------------------------------- single-query calls --
def test_query_forms_inside_a_namespace(idxmod, cuda):
    n = 700  # three pages on one shard, the last one partial
    A = vectors(n, 5)
    meta = [{"bucket": i % 3, "tag": "even" if i % 2 == 0 else "odd"} for i in range(n)]
    ix = idxmod.Index("forms", dimension=DIM, capacity=64, device=cuda)
    fill(ix, "a", A, meta=meta)
    fill(ix, "", vectors(20, 6))
    # a namespace that does not exist: no matches, its name echoed
    assert ix.query(vector=A[0].tolist(), top_k=3, namespace="nobody") == {"matches": [], "namespace": "nobody"}
    assert ix.fetch(["v1"], namespace="nobody") == {"vectors": {}, "namespace": "nobody"}
    assert ix.delete(ids=["v1"], namespace="nobody") == {} and ix.delete(delete_all=True, namespace="nobody") == {}
    # query by id: the id's own vector is the query
    r = ix.query(id="v650", top_k=4, namespace="a", include_metadata=True)
    o, _ = ranking64(A, A[650])
    assert [m["id"] for m in r["matches"]] == [f"v{i}" for i in o[:4]] and r["matches"][0]["metadata"] == meta[650]
    assert ix.query(id="v650", top_k=4) == {"matches": [], "namespace": ""}  # "" has no such id
    # metadata filter against a float64 ranking of the namespace's eligible vectors
    q = vectors(4, 77)[1]
    elig = np.array([m["bucket"] == 1 and m["tag"] == "odd" for m in meta])
    o, s = ranking64(A, q)
    o = [i for i in o if elig[i]]
    top = s[o[:11]]
    assert (top[:-1] - top[1:]).min() > 1e-5  # the data: neighbouring scores differ by far more than f32 rounding
    r = ix.query(vector=q.tolist(), top_k=10, namespace="a", filter={"bucket": 1, "tag": {"$eq": "odd"}})
    assert [m["id"] for m in r["matches"]] == [f"v{i}" for i in o[:10]]
    np.testing.assert_allclose([m["score"] for m in r["matches"]], s[o[:10]], rtol=0, atol=1e-5)
    assert ix.query(vector=q.tolist(), top_k=10, namespace="a", filter={"bucket": 9})["matches"] == []
    few = ix.query(vector=q.tolist(), top_k=256, namespace="a", filter={"bucket": 1, "tag": "odd"})["matches"]
    assert len(few) == min(256, int(elig.sum()))
    ix.close()


def test_euclidean_scores_are_reported_as_squared_distances(idxmod, cuda):
    A = vectors(300, 8)
    ix = idxmod.Index("euc", dimension=DIM, metric="euclidean", capacity=64, device=cuda)
    fill(ix, "a", A)
    q = vectors(3, 9)[0]
    o, s = ranking64(A, q, "euclidean")
    r = ix.query(vector=q.tolist(), top_k=6, namespace="a")["matches"]
    assert [m["id"] for m in r] == [f"v{i}" for i in o[:6]]
    np.testing.assert_allclose([m["score"] for m in r], s[o[:6]], rtol=1e-4)
    assert all(x["score"] <= y["score"] for x, y in zip(r, r[1:]))
    own = ix.query(id="v5", top_k=1, namespace="a")["matches"][0]
    assert own["id"] == "v5" and 0.0 <= own["score"] < 1e-3
    ix.close()


# --------------------------------------------------------------- batched calls --
def test_query_batch_in_a_namespace_equals_the_single_queries(idxmod, cuda):
    import torch

    n = 600
    A = vectors(n, 11)
    meta = [{"k": i % 4} for i in range(n)]
    ix = idxmod.Index("batch", dimension=DIM, dtype="float16", capacity=64, device=cuda)
    fill(ix, "a", A, meta=meta)
    Q = vectors(9, 12)
    for kw in ({}, {"filter": {"k": {"$in": [1, 2]}}}):
        for mode in ("auto", "scan"):
            got = ix.query_batch(torch.from_numpy(Q), top_k=10, namespace="a", mode=mode, **kw)
            assert all(r["namespace"] == "a" for r in got)
            for qi in range(len(Q)):
                assert matches(got[qi]) == matches(ix.query(vector=Q[qi].tolist(), top_k=10, namespace="a", **kw)), (kw, mode, qi)
    vals = ix.query_batch(Q[:2], top_k=3, namespace="a", include_values=True)
    for r in vals:
        for m in r["matches"]:
            np.testing.assert_allclose(m["values"], A[int(m["id"][1:])], rtol=0, atol=4e-3)  # f16 storage: 2^-11 of values up to ~4, twice over
    for mode in ("mfma", "mfma_masked"):
        with pytest.raises(ValueError, match="namespace"):
            ix.query_batch(Q, top_k=10, namespace="a", mode=mode)
    assert ix.query_batch(Q[:2], top_k=3, namespace="nobody") == [{"matches": [], "namespace": "nobody"}] * 2
    ix.close()


# ----------------------------------------------------------------------- delete --
@pytest.mark.parametrize("shards", [1, 3])
def test_delete_inside_a_namespace(idxmod, cuda, shards):
    span = 256 * shards
    n = span + 100  # two pages; deleting 150 crosses back over the page edge
    A, B, D = vectors(n, 21), vectors(300, 22), vectors(40, 23)
    meta = [{"drop": i % 7 == 0} for i in range(n)]
    ix = idxmod.Index("del", dimension=DIM, capacity=64, device=cuda, shards=shards)
    fill(ix, "a", A, meta=meta)
    fill(ix, "b", B)
    fill(ix, "", D)
    na = ix._ns["a"]
    assert len(na.pages) == 2
    qb = B[3].tolist()
    before_b, before_d = matches(ix.query(vector=qb, top_k=10, namespace="b")), matches(ix.query(vector=qb, top_k=10))
    gone = [f"v{i}" for i in list(range(0, 140)) + list(range(n - 10, n))]
    assert ix.delete(ids=gone + ["v0", "unknown"], namespace="a") == {}
    alive = [i for i in range(n) if f"v{i}" not in set(gone)]
    assert ix.describe_index_stats()["namespaces"]["a"]["vector_count"] == len(alive) == n - 150
    assert len(na.pages) == 1  # the emptied page went back to the free list
    got = ix.fetch([f"v{i}" for i in alive], namespace="a")["vectors"]
    assert len(got) == len(alive)
    for i in alive:  # every remaining id still fetches its own values
        np.testing.assert_allclose(got[f"v{i}"]["values"], A[i], rtol=0, atol=1e-5)
    assert ix.fetch(gone[:5], namespace="a")["vectors"] == {}
    q = A[alive[17]].tolist()
    o, _ = ranking64(A[alive], q)
    assert [m["id"] for m in ix.query(vector=q, top_k=8, namespace="a")["matches"]] == [f"v{alive[i]}" for i in o[:8]]
    # by filter
    ix.delete(filter={"drop": True}, namespace="a")
    alive = [i for i in alive if not meta[i]["drop"]]
    assert ix.describe_index_stats()["namespaces"]["a"]["vector_count"] == len(alive)
    o, _ = ranking64(A[alive], q)
    assert [m["id"] for m in ix.query(vector=q, top_k=8, namespace="a")["matches"]] == [f"v{alive[i]}" for i in o[:8]]
    # "b" and "" never noticed
    assert matches(ix.query(vector=qb, top_k=10, namespace="b")) == before_b
    assert matches(ix.query(vector=qb, top_k=10)) == before_d
    assert len(ix) == 40 and ix.fetch(["v0"])["vectors"]["v0"]["id"] == "v0"
    # delete_all: the namespace disappears, and the next upsert reuses its pages without growing the pool
    cap, high = ix.pool.capacity_per_shard, ix._alloc.high_water
    free_before = ix._alloc.free_pages
    ix.delete(delete_all=True, namespace="b")
    st = ix.describe_index_stats()
    assert "b" not in st["namespaces"] and st["total_vector_count"] == len(alive) + 40
    assert ix.query(vector=qb, top_k=3, namespace="b") == {"matches": [], "namespace": "b"}
    fill(ix, "c", B)
    assert ix.pool.capacity_per_shard == cap and ix._alloc.high_water == high
    assert not set(ix._ns["c"].pages) & set(na.pages) and max(ix._ns["c"].pages) < high
    assert ix._alloc.free_pages == free_before  # "c" holds as many pages as "b" gave back
    assert matches(ix.query(vector=qb, top_k=10, namespace="c")) == before_b
    # deleting the last vectors of a namespace removes it as well
    ix.delete(ids=[f"v{i}" for i in alive], namespace="a")
    assert "a" not in ix.describe_index_stats()["namespaces"] and "a" not in ix._ns
    ix.close()


# ----------------------------------------------------------------------- growth --
def test_pool_growth_keeps_results(idxmod, cuda):
    A, B = vectors(500, 31), vectors(1500, 32)
    ix = idxmod.Index("grow", dimension=DIM, capacity=64, device=cuda)
    fill(ix, "a", A)
    cap0 = ix.pool.capacity_per_shard
    Q = vectors(5, 33)
    before = [matches(ix.query(vector=q.tolist(), top_k=10, namespace="a")) for q in Q]
    fill(ix, "b", B)  # 6 more pages: past the pool's first 4
    assert ix.pool.capacity_per_shard > cap0 and ix.pool.capacity_per_shard % 256 == 0
    assert [matches(ix.query(vector=q.tolist(), top_k=10, namespace="a")) for q in Q] == before
    o, _ = ranking64(B, Q[0])
    assert [m["id"] for m in ix.query(vector=Q[0].tolist(), top_k=10, namespace="b")["matches"]] == [f"v{i}" for i in o[:10]]
    fill(ix, "a", vectors(900, 34), ids=ids_of(900, "w"))  # "a" itself grows over non-adjacent pages
    pa = ix._ns["a"].pages
    assert len(pa) == 6 and pa[2] != pa[1] + 1  # "b" sits between its first pages and its later ones
    o, _ = ranking64(np.concatenate([A, vectors(900, 34)]), Q[1])
    names = ids_of(500) + ids_of(900, "w")
    assert [m["id"] for m in ix.query(vector=Q[1].tolist(), top_k=10, namespace="a")["matches"]] == [names[i] for i in o[:10]]
    ix.close()


# ----------------------------------------------------------------------- shards --
def test_three_shards_answer_as_one(idxmod, cuda):
    A, B = vectors(900, 41), vectors(300, 42)
    meta = [{"m": i % 5} for i in range(900)]
    out = []
    for shards in (1, 3):
        ix = idxmod.Index(f"sh{shards}", dimension=DIM, dtype="bfloat16", capacity=64, device=cuda, shards=shards)
        fill(ix, "a", A, meta=meta)
        fill(ix, "b", B)
        ix.delete(ids=[f"v{i}" for i in range(100, 400, 3)], namespace="a")
        Q = vectors(6, 43)
        res = [matches(ix.query(vector=q.tolist(), top_k=20, namespace="a")) for q in Q]
        res += [matches(ix.query(vector=q.tolist(), top_k=20, namespace="a", filter={"m": {"$ne": 2}})) for q in Q]
        res += [matches(r) for r in ix.query_batch(Q, top_k=20, namespace="b")]
        out.append(res)
        ix.close()
    # the same ids and score bits; positions differ between the two (the delete plan pairs rows per shard)
    assert out[0] == out[1]


# ---------------------------------------------------------------- save and load --
def test_save_and_load_round_trip_namespaces_into_another_shard_count(idxmod, cuda, tmp_path):
    A, B, D = vectors(600, 51), vectors(300, 52), vectors(40, 53)
    ix = idxmod.Index("snap", dimension=DIM, dtype="float16", capacity=64, device=cuda, shards=3)
    fill(ix, "a", A[:300], meta=[{"i": i} for i in range(300)])
    fill(ix, "b", B)
    fill(ix, "a", A[300:], ids=ids_of(600)[300:])  # "a"'s pages are not consecutive
    fill(ix, "", D)
    ix.delete(ids=["v5", "v6"], namespace="a")
    Q = vectors(4, 54)

    def snapshot(x):
        out = []
        for ns in ("a", "b", ""):
            out += [matches(x.query(vector=q.tolist(), top_k=10, namespace=ns)) for q in Q]
        out.append(x.describe_index_stats()["namespaces"])
        out.append(x.query(id="v9", top_k=1, namespace="a", include_metadata=True)["matches"][0]["metadata"])
        return out

    want = snapshot(ix)
    ix.save(str(tmp_path / "two"))
    man = json.load(open(tmp_path / "two" / "manifest.json"))
    assert man["format"] == 2 and [s["name"] for s in man["namespaces"]] == ["a", "b"]
    ix.close()
    back = idxmod.Index.load(str(tmp_path / "two"), device=cuda, shards=2)
    assert snapshot(back) == want
    v = back.fetch(["v599"], namespace="a")["vectors"]["v599"]["values"]
    np.testing.assert_allclose(v, A[599], rtol=0, atol=4e-3)  # f16 storage: 2^-11 of values up to ~4, twice over
    # without a named namespace the snapshot is format 1, as ever
    back.delete(delete_all=True, namespace="a")
    back.delete(delete_all=True, namespace="b")
    back.save(str(tmp_path / "plain"))
    man = json.load(open(tmp_path / "plain" / "manifest.json"))
    assert man["format"] == 1 and "namespaces" not in man
    assert sorted(os.listdir(tmp_path / "plain")) == ["manifest.json", "norms.npy", "rows.npy"]
    back.close()
    again = idxmod.Index.load(str(tmp_path / "plain"), device=cuda)
    assert [matches(again.query(vector=q.tolist(), top_k=10)) for q in Q] == want[8:12]
    assert again.describe_index_stats()["namespaces"] == {"": {"vector_count": 40}}
    again.close()


# ---------------------------------------------------------------------- service --
def _jpeg(seed, w=224, h=224):
    from PIL import Image

    arr = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="JPEG", quality=85)
    return b.getvalue()


def test_service_routes_take_a_namespace(cuda, monkeypatch):
    from fastapi.testclient import TestClient

    cfg = import_pkg("config").Config
    name = "namespace-service"
    monkeypatch.setattr(cfg, "INDEX_NAME", name)
    svc = TestClient(import_pkg("service").app)
    try:
        a, b, c = _jpeg(601), _jpeg(602, 256, 200), _jpeg(603, 200, 256)
        r = svc.post("/push_image", files={"file": ("a.jpg", a, "image/jpeg")}, data={"namespace": "alice"})
        assert r.status_code == 200
        pa = r.json()
        r = svc.post("/push_images", files=[("files", ("b.jpg", b, "image/jpeg")), ("files", ("c.jpg", c, "image/jpeg"))],
                     data={"namespace": "alice"})
        assert r.status_code == 200 and len(r.json()) == 2
        pb = r.json()[0]
        r = svc.post("/push_image", files={"file": ("d.jpg", a, "image/jpeg")})  # the same image, default namespace
        pd = r.json()
        ix = import_pkg("service").index()
        assert ix.describe_index_stats()["namespaces"] == {"": {"vector_count": 1}, "alice": {"vector_count": 3}}
        q = {"file": ("q.jpg", a, "image/jpeg")}
        r = svc.post("/search_image", files=q, data={"namespace": "alice"})
        assert r.status_code == 200 and len(r.json()) == 3 and r.json()[0] == pa["signed_url"]
        r = svc.post("/search_image", files={"file": ("q.jpg", b, "image/jpeg")},
                     data={"namespace": "alice", "filter": json.dumps({"filename": "b.jpg"})})
        assert r.json() == [pb["signed_url"]]
        assert svc.post("/search_image", files=q, data={"namespace": "bob"}).json() == []
        assert svc.post("/search_image", files=q).json() == [pd["signed_url"]]  # absent = ""
        # delete in the wrong namespace removes nothing; in the right one, the image
        assert svc.post("/delete_images", json={"ids": [pa["file_id"]]}).json() == {"deleted_count": 0}
        assert svc.post("/delete_images", json={"ids": [pa["file_id"]], "namespace": "bob"}).json() == {"deleted_count": 0}
        assert svc.post("/delete_images", json={"ids": [pa["file_id"]], "namespace": "alice"}).json() == {"deleted_count": 1}
        assert svc.post("/delete_images", json={"ids": [pa["file_id"]], "namespace": 3}).status_code == 422
        r = svc.post("/search_image", files=q, data={"namespace": "alice"})
        assert len(r.json()) == 2 and pa["signed_url"] not in r.json()
        assert svc.post("/search_image", files=q).json() == [pd["signed_url"]]
    finally:
        ix = import_pkg("ingesting.utils")._indexes.pop(name, None)
        if ix is not None:
            ix.close()
