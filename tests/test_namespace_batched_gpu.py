"""``Index(..., paged_search="mfma")`` on the GPU: ``query_batch`` in a named namespace takes all four
modes, hands them to the batched MFMA search over the namespace's pages, and returns what the
per-query ``query`` (the paged scan) returns: the same ids and the same score bits."""
import numpy as np
import pytest

from conftest import import_pkg

pytestmark = pytest.mark.gpu

DIM = 64
MODES = ("auto", "scan", "mfma", "mfma_masked")


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


_DATA = {}


def vectors(n, seed, dim=DIM):
    key = (n, seed, dim)
    if key not in _DATA:
        _DATA[key] = np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)
    return _DATA[key]


def fill(ix, ns, X, meta=None, prefix="v", step=2000):
    import torch

    ids = [f"{prefix}{i}" for i in range(len(X))]
    for i in range(0, len(X), step):
        ix.upsert_tensor(ids[i:i + step], torch.from_numpy(X[i:i + step]).cuda(), None if meta is None else meta[i:i + step],
                         namespace=ns)


def matches(res):
    return [(m["id"], np.float32(m["score"]).view(np.uint32).item()) for m in res["matches"]]


def check_batch_equals_queries(ix, ns, Q, k, flt=None):
    """query_batch under every mode against the per-query query(), as (id, score bits)."""
    want = [matches(ix.query(vector=q.tolist(), top_k=k, namespace=ns, filter=flt)) for q in Q]
    assert all(len(w) > 0 for w in want)
    for mode in MODES:
        got = ix.query_batch(Q, top_k=k, mode=mode, namespace=ns, filter=flt)
        assert all(r["namespace"] == ns for r in got)
        assert [matches(r) for r in got] == want, mode


@pytest.mark.parametrize("dtype,metric,filt", [("float16", "cosine", "native"), ("bfloat16", "euclidean", "metric")])
def test_query_batch_in_a_namespace_equals_per_query_results_under_every_mode(idxmod, cuda, dtype, metric, filt):
    n = 4096 + 3 * 256 + 77  # two stages of the batched search, a partial last page
    A = vectors(n, 1)
    if metric != "cosine":
        A = A * (2.0 ** np.random.default_rng(2).uniform(-2, 2, n)).astype(np.float32)[:, None]
    meta = [{"bucket": i % 3} for i in range(n)]
    ix = idxmod.Index("nsb", dimension=DIM, metric=metric, dtype=dtype, capacity=256, device=cuda, filter=filt, paged_search="mfma")
    fill(ix, "other", vectors(600, 3), prefix="o")  # pages handed out before and between alice's
    fill(ix, "alice", A[:3000], meta=meta[:3000])
    fill(ix, "other2", vectors(300, 4), prefix="p")
    fill(ix, "alice", A, meta=meta)  # the first 3000 ids again (overwritten in place) and the rest: a non-monotonic page list
    assert ix.pool.filter == filt
    Q = vectors(9, 5)
    check_batch_equals_queries(ix, "alice", Q, 10)
    check_batch_equals_queries(ix, "alice", Q, 10, flt={"bucket": 1})
    if metric == "euclidean":  # reported scores are squared distances, ascending
        r = ix.query_batch(Q[:2], top_k=5, mode="mfma", namespace="alice")
        for q, res in zip(Q[:2], r):
            sc = [m["score"] for m in res["matches"]]
            assert sc == sorted(sc) and sc[0] >= 0.0
            best = int(res["matches"][0]["id"][1:])
            d2 = ((A.astype(np.float64) - q[None].astype(np.float64)) ** 2).sum(1)
            # bf16 storage moves a vector by at most 2^-9 of its norm, hence each distance by as much:
            # the reported best is within twice that of the float64 best
            slack = 2 * 2.0 ** -9 * np.linalg.norm(A.astype(np.float64), axis=1).max()
            assert np.sqrt(d2[best]) - np.sqrt(d2.min()) <= slack
    ix.close()


def test_colliding_ids_delete_and_snapshot_round_trip(idxmod, cuda, tmp_path):
    n = 4096 + 700
    A, B, D = vectors(n, 7), vectors(n, 8), vectors(300, 9)
    ix = idxmod.Index("nsb2", dimension=DIM, dtype="float16", capacity=256, device=cuda, paged_search="mfma")
    plain = idxmod.Index("nsb2-plain", dimension=DIM, dtype="float16", capacity=256, device=cuda)
    fill(ix, "", D)
    fill(plain, "", D)
    fill(ix, "a", A)
    fill(ix, "b", B)  # the same ids, other vectors
    Q = np.concatenate([A[[5, 4500]], B[[5, 4500]], vectors(5, 10)])
    for ns, X in (("a", A), ("b", B)):
        check_batch_equals_queries(ix, ns, Q, 10)
    ra = ix.query_batch(Q[:4], top_k=3, mode="mfma", namespace="a")
    rb = ix.query_batch(Q[:4], top_k=3, mode="mfma", namespace="b")
    assert [r["matches"][0]["id"] for r in ra[:2]] == ["v5", "v4500"] and all(abs(r["matches"][0]["score"] - 1) < 1e-3 for r in ra[:2])
    assert [r["matches"][0]["id"] for r in rb[2:]] == ["v5", "v4500"] and all(abs(r["matches"][0]["score"] - 1) < 1e-3 for r in rb[2:])
    assert all(r["matches"][0]["score"] < 0.9 for r in ra[2:] + rb[:2])  # neither sees the other's vectors
    # "" is what an index without namespaces answers
    assert [matches(r) for r in ix.query_batch(D[:9], top_k=7)] == [matches(r) for r in plain.query_batch(D[:9], top_k=7)]
    # delete: rows move into the holes and whole pages go back to the pool
    gone = [f"v{i}" for i in range(100, 100 + 1500)]
    ix.delete(ids=gone, namespace="a")
    check_batch_equals_queries(ix, "a", Q, 10)
    got = {m["id"] for r in ix.query_batch(Q, top_k=50, mode="mfma", namespace="a") for m in r["matches"]}
    assert not got & set(gone)
    # save / load: the keyword is load's too, and the snapshot format is the default index's
    path = str(tmp_path / "snap")
    ix.save(path)
    back = idxmod.Index.load(path, device=cuda, paged_search="mfma")
    for ns in ("a", "b"):
        want = [matches(r) for r in ix.query_batch(Q, top_k=10, mode="scan", namespace=ns)]
        for mode in MODES:
            assert [matches(r) for r in back.query_batch(Q, top_k=10, mode=mode, namespace=ns)] == want, (ns, mode)
    default = idxmod.Index.load(path, device=cuda)  # the same files load without the keyword
    assert [matches(r) for r in default.query_batch(Q, top_k=10, namespace="a")] == \
        [matches(r) for r in ix.query_batch(Q, top_k=10, mode="scan", namespace="a")]
    with pytest.raises(ValueError, match="namespace"):
        default.query_batch(Q, top_k=10, mode="mfma", namespace="a")
    for x in (ix, plain, back, default):
        x.close()


def test_a_default_index_still_refuses_mfma_in_a_namespace(idxmod, cuda):
    ix = idxmod.Index("nsb3", dimension=DIM, dtype="float16", capacity=256, device=cuda)
    fill(ix, "a", vectors(300, 11))
    for mode in ("mfma", "mfma_masked"):
        with pytest.raises(ValueError, match="namespace") as e:
            ix.query_batch(vectors(9, 5), top_k=5, mode=mode, namespace="a")
        assert "paged_search" in str(e.value)  # it says how to enable the path
    assert len(ix.query_batch(vectors(9, 5), top_k=5, mode="auto", namespace="a")) == 9
    ix.close()
