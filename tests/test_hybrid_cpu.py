"""Sparse-dense hybrid without a GPU: the validation of sparse values, the float32 model of the
device's sparse term, the client-side convex weighting, the C ABI's new calls (declared, exported,
bound, refusing a NULL handle before any device call), and a manifest that gains no key unless the
feature is on."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO, import_pkg

CALLS = ["rc_index_sparse_enable", "rc_index_sparse_width", "rc_index_sparse_write", "rc_sharded_sparse_enable",
         "rc_sharded_sparse_write", "rc_index_search_hybrid", "rc_index_search_pages_hybrid", "rc_sharded_search_hybrid",
         "rc_sharded_search_pages_hybrid", "rc_index_scores_hybrid"]


@pytest.fixture(scope="module")
def sv():
    return import_pkg("sparsevalues")


@pytest.fixture(scope="module")
def L():
    return import_pkg("_lib")


@pytest.fixture(scope="module")
def lib(L):
    return L.load()


def header():
    return open(os.path.join(REPO, "include", "retrieval_core.h")).read()


# ------------------------------------------------------------------ validation --
def test_width_is_zero_or_an_integer_up_to_1024(sv):
    for ok in (0, 1, 64, 1024, np.int64(5)):
        assert sv.validate_width(ok) == int(ok)
    for bad in (-1, 1025, 1.0, "8", None, True, [4]):
        with pytest.raises(ValueError, match="sparse_max_nnz"):
            sv.validate_width(bad)


def test_normalize_accepts_and_sorts(sv):
    idx, val = sv.normalize({"indices": [7, 0, 2 ** 32 - 2], "values": [1.5, -2, 3]}, 4)
    assert idx.dtype == np.uint32 and val.dtype == np.float32
    assert idx.tolist() == [0, 7, 2 ** 32 - 2] and val.tolist() == [-2.0, 1.5, 3.0]
    assert sv.normalize(None, 4) is None
    assert sv.normalize({"indices": [], "values": []}, 4) is None  # an empty pair means "none"
    assert sv.normalize({"indices": [], "values": []}, 0) is None  # ... on an index without the feature too
    full = sv.normalize({"indices": list(range(4)), "values": [1.0] * 4}, 4)  # exactly the limit
    assert full[0].tolist() == [0, 1, 2, 3]
    n = sv.normalize({"indices": np.array([3, 1]), "values": np.array([1.0, 2.0], np.float32)}, 4)  # arrays are fine
    assert n[0].tolist() == [1, 3] and n[1].tolist() == [2.0, 1.0]
    assert sv.to_dict(n) == {"indices": [1, 3], "values": [2.0, 1.0]}


@pytest.mark.parametrize("bad", [
    {"indices": [1, 1], "values": [1.0, 2.0]},          # repeated
    {"indices": [2 ** 32 - 1], "values": [1.0]},        # the padding value
    {"indices": [2 ** 32], "values": [1.0]},            # out of range
    {"indices": [-1], "values": [1.0]},
    {"indices": [1.0], "values": [1.0]},                # not an integer
    {"indices": [True], "values": [1.0]},
    {"indices": [1, 2], "values": [1.0]},               # lengths differ
    {"indices": [1], "values": [float("nan")]},
    {"indices": [1], "values": [float("inf")]},
    {"indices": [1], "values": [1e39]},                 # overflows float32
    {"indices": [1], "values": ["1.0"]},
    {"indices": [1, 2, 3], "values": [1.0, 2.0, 3.0]},  # more than the limit of 2
    {"indices": [1]},
    {"indices": [1], "values": [1.0], "extra": 0},
    [[1], [1.0]],
    "x",
    {"indices": 3, "values": 1.0},
])
def test_normalize_rejects(sv, bad):
    with pytest.raises(ValueError):
        sv.normalize(bad, 2)


def test_values_on_an_index_without_the_feature_are_refused(sv):
    with pytest.raises(ValueError, match="sparse_max_nnz"):
        sv.normalize({"indices": [1], "values": [1.0]}, 0)


def test_csr(sv):
    a = sv.normalize({"indices": [5, 1], "values": [1, 2]}, 4)
    off, idx, val = sv.csr([a, None, a], np.int32)
    assert off.dtype == np.int32 and off.tolist() == [0, 2, 2, 4]
    assert idx[:4].tolist() == [1, 5, 1, 5] and val[:4].tolist() == [2.0, 1.0, 2.0, 1.0]
    off, idx, val = sv.csr([None])
    assert off.tolist() == [0, 0] and idx.size >= 1 and val.size >= 1  # never a zero-length buffer


# ------------------------------------------------------------------- model_term --
def test_model_term_is_the_sequential_unfused_float32_sum(sv):
    # chosen so the order and the rounding of each product show: f32(f32(1e8 * 1) + f32(1 * 1)) - 1e8 == 0
    t = sv.model_term([1, 2, 3], [1e8, 1.0, -1e8], [1, 2, 3], [1.0, 1.0, 1.0])
    assert isinstance(t, np.float32) and t == np.float32(0.0)
    t = sv.model_term([3, 1, 2], [-1e8, 1e8, 1.0], [1, 2, 3], [1.0, 1.0, 1.0])  # stored order does not matter: index order does
    assert t == np.float32(0.0)
    assert sv.model_term([1, 3], [1e8, -1e8], [1, 2, 3], [1.0, 1.0, 1.0]) == np.float32(0.0)
    assert sv.model_term([2, 9], [1.0, 5.0], [1, 2, 3], [1.0, 0.5, 1.0]) == np.float32(0.5)  # only shared indices count
    z = sv.model_term([], [], [1], [1.0])
    assert z == 0.0 and not np.signbit(z)  # +0.0
    assert sv.model_term([4], [2.0], [], []) == 0.0
    # each product is rounded to float32 before it is added (unfused)
    a, b = np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -12)
    assert sv.model_term([0], [a], [0], [b]) == np.float32(a * b)


def test_model_term_agrees_with_float64_within_the_bound(sv):
    rng = np.random.default_rng(0)
    for nnz in (1, 7, 64, 1024):
        idx = rng.choice(2 ** 32 - 1, nnz, replace=False).astype(np.uint32)
        v = (rng.standard_normal(nnz) * 10 ** rng.uniform(-3, 3, nnz)).astype(np.float32)
        w = (rng.standard_normal(nnz) * 10 ** rng.uniform(-3, 3, nnz)).astype(np.float32)
        t = sv.model_term(idx, v, idx[::-1].copy(), w[::-1].copy())
        prod = v.astype(np.float64) * w.astype(np.float64)
        assert abs(float(t) - prod.sum()) <= nnz * 2.0 ** -23 * np.abs(prod).sum(), nnz


# ------------------------------------------------------------------ convex scale --
def test_hybrid_convex_scale(sv):
    d, s = sv.hybrid_convex_scale([1.0, -2.0], {"indices": [3, 9], "values": [4.0, 8.0]}, 0.25)
    assert d == [0.25, -0.5] and s == {"indices": [3, 9], "values": [3.0, 6.0]}
    d, s = sv.hybrid_convex_scale([1.0], {"indices": [1], "values": [2.0]}, 1)  # dense only
    assert d == [1.0] and s["values"] == [0.0]
    d, s = sv.hybrid_convex_scale([1.0], {"indices": [1], "values": [2.0]}, 0)  # sparse only
    assert d == [0.0] and s["values"] == [2.0]
    for bad in (-0.1, 1.1, "0.5", None, True):
        with pytest.raises(ValueError, match="alpha"):
            sv.hybrid_convex_scale([1.0], {"indices": [1], "values": [2.0]}, bad)
    with pytest.raises(ValueError):
        sv.hybrid_convex_scale([1.0], {"indices": [1]}, 0.5)


# ----------------------------------------------------------------------- the ABI --
def test_the_new_calls_are_declared_exported_and_bound(L, lib):
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in CALLS:
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert hasattr(raw, name), name
        assert name in L.SIGNATURES and name not in lib.rc_missing_symbols
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    # the hybrid searches take their deep twins' arguments plus the three CSR arrays
    for a, b in [("rc_index_search_hybrid", "rc_index_search_deep"), ("rc_index_search_pages_hybrid", "rc_index_search_pages_deep"),
                 ("rc_sharded_search_hybrid", "rc_sharded_search_deep"), ("rc_sharded_search_pages_hybrid", "rc_sharded_search_pages_deep")]:
        assert len(L.SIGNATURES[a][1]) == len(L.SIGNATURES[b][1]) + 3


def test_the_abi_version_and_the_limit(L, lib, sv):
    assert lib.rc_abi_version() == 1
    assert re.search(r"#define RC_ABI_VERSION 1\b", header())
    defs = dict(re.findall(r"#define (RC_[A-Z_]+) (\d+)", header()))
    assert int(defs["RC_SPARSE_MAX_NNZ"]) == L.RC_SPARSE_MAX_NNZ == sv.MAX_NNZ == 1024
    assert sv.PAD == 2 ** 32 - 1


def test_the_new_calls_refuse_a_null_handle(L, lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    bad = L.RC_ERR_INVALID
    assert lib.rc_index_sparse_enable(None, 4, None) == bad
    assert b"null index" in lib.rc_last_error()
    w = ctypes.c_int()
    assert lib.rc_index_sparse_width(None, ctypes.byref(w)) == bad
    assert lib.rc_index_sparse_write(None, p, p, p, p, 1, None) == bad
    assert lib.rc_sharded_sparse_enable(None, 4) == bad
    assert lib.rc_sharded_sparse_write(None, p, p, p, p, 1) == bad
    assert lib.rc_index_search_hybrid(None, p, 1, 10, 5, None, p, p, p, p, p, None) == bad
    assert lib.rc_index_search_pages_hybrid(None, p, 1, 0, 10, 5, None, p, p, p, p, p, None) == bad
    assert lib.rc_sharded_search_hybrid(None, p, 1, 10, 5, None, p, p, p, p, p, None) == bad
    assert lib.rc_sharded_search_pages_hybrid(None, p, 1, 0, 10, 5, None, p, p, p, p, p, None) == bad
    assert lib.rc_index_scores_hybrid(None, p, -1, 10, p, p, p, p, None) == bad
    assert b"null index" in lib.rc_last_error()


# ------------------------------------------------------------- the Python surface --
def test_the_constructor_validates_before_anything_is_made():
    idxmod = import_pkg("index")
    for bad in (-1, 1025, 2.0, "4", None, True):
        with pytest.raises(ValueError, match="sparse_max_nnz"):
            idxmod.Index("x", dimension=8, metric="dotproduct", sparse_max_nnz=bad)
    for metric in ("cosine", "euclidean"):  # as in Pinecone: sparse values are dotproduct-only
        with pytest.raises(ValueError, match="dotproduct"):
            idxmod.Index("x", dimension=8, metric=metric, sparse_max_nnz=4)
    assert inspect.signature(idxmod.Index.__init__).parameters["sparse_max_nnz"].default == 0
    assert "sparse_vector" in inspect.signature(idxmod.Index.query).parameters
    assert "sparse_vectors" in inspect.signature(idxmod.Index.query_batch).parameters
    assert "sparse_values" in inspect.signature(idxmod.Index.upsert_tensor).parameters
    for cls in (idxmod.DeviceIndex, idxmod.ShardSet):
        for name in ("sparse_enable", "sparse_write", "search_hybrid", "search_pages_hybrid", "scores_hybrid"):
            assert callable(getattr(cls, name)), (cls, name)


def test_the_manifest_gains_no_key_unless_the_feature_is_on():
    """At source level: ``save`` writes "sparse_max_nnz" and the sparse files only under
    ``if self.sparse_max_nnz`` — an index made with the default writes the manifest it always wrote."""
    idxmod = import_pkg("index")
    src = inspect.getsource(idxmod.Index.save)
    assert len(re.findall(r'"sparse_max_nnz"', src)) == 1
    assert re.search(r'if self\.sparse_max_nnz:[^\n]*\n\s+manifest\["sparse_max_nnz"\] = self\.sparse_max_nnz', src)
    helper = inspect.getsource(idxmod.Index._save_sparse)
    assert re.search(r"if not self\.sparse_max_nnz:\s*\n\s+return", helper)
    assert helper.index("return") < helper.index("np.save")
    load = inspect.getsource(idxmod.Index.load)
    assert '"sparse_max_nnz" in man' in load


def test_retriever_search_passes_the_sparse_vector_only_when_given():
    utils = import_pkg("retriever.utils")
    seen = []

    class Probe:
        def query(self, **kw):
            seen.append(kw)
            return {"matches": [{"id": "a"}]}

    assert utils.search(Probe(), [1.0], 3) == ["a"]
    assert "sparse_vector" not in seen[-1]
    sp = {"indices": [1], "values": [2.0]}
    utils.search(Probe(), [1.0], 3, sparse_vector=sp)
    assert seen[-1]["sparse_vector"] is sp
