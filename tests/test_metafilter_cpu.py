"""Metadata filters (``metafilter``): the filter language, its stated semantics, the bitmap
layout the masked search takes, and the masked sharded entry points' argument validation.

No GPU: the predicate and the bitmap are host-side, and the two library calls below return
``RC_ERR_INVALID`` before touching a device.
"""
import ctypes

import numpy as np
import pytest

from conftest import import_pkg


@pytest.fixture(scope="module")
def mf():
    return import_pkg("metafilter")


def ok(mf, flt, md):
    return mf.compile_filter(flt)(md)


MD = {"album": 3, "owner": "ann", "score": 2.5, "public": True, "tag": ["cat", "pet"], "n": 0}


@pytest.mark.parametrize("flt,want", [
    ({"album": {"$eq": 3}}, True),
    ({"album": {"$eq": 4}}, False),
    ({"album": 3}, True),                      # a bare value means $eq
    ({"owner": "ann"}, True),
    ({"owner": "bob"}, False),
    ({"album": {"$ne": 3}}, False),
    ({"album": {"$ne": 4}}, True),
    ({"album": {"$gt": 2}}, True),
    ({"album": {"$gt": 3}}, False),
    ({"album": {"$gte": 3}}, True),
    ({"album": {"$gte": 3.5}}, False),
    ({"album": {"$lt": 4}}, True),
    ({"album": {"$lt": 3}}, False),
    ({"album": {"$lte": 3}}, True),
    ({"album": {"$lte": 2}}, False),
    ({"score": {"$gt": 2}}, True),             # int operand against a float field
    ({"album": {"$in": [1, 3]}}, True),
    ({"album": {"$in": [1, 2]}}, False),
    ({"album": {"$in": []}}, False),
    ({"album": {"$nin": [1, 2]}}, True),
    ({"album": {"$nin": [3]}}, False),
    ({"album": {"$exists": True}}, True),
    ({"album": {"$exists": False}}, False),
    ({"nope": {"$exists": False}}, True),
    ({"nope": {"$exists": True}}, False),
    ({"album": {"$gte": 2, "$lt": 4}}, True),  # several operators of one field: AND
    ({"album": {"$gte": 2, "$lt": 3}}, False),
    ({}, True),
])
def test_every_operator(mf, flt, want):
    assert ok(mf, flt, MD) is want


def test_implicit_and_over_fields(mf):
    assert ok(mf, {"album": 3, "owner": "ann"}, MD)
    assert not ok(mf, {"album": 3, "owner": "bob"}, MD)
    assert not ok(mf, {"album": 4, "owner": "ann"}, MD)


def test_nested_and_or(mf):
    f = {"$or": [{"album": 9}, {"$and": [{"owner": "ann"}, {"score": {"$lt": 3}}]}]}
    assert ok(mf, f, MD)
    assert not ok(mf, f, {**MD, "score": 5})
    assert ok(mf, f, {"album": 9})
    g = {"$and": [{"$or": [{"album": 1}, {"album": 3}]}, {"public": True}], "owner": "ann"}
    assert ok(mf, g, MD)
    assert not ok(mf, g, {**MD, "public": False})
    assert not ok(mf, g, {**MD, "owner": "bob"})
    assert not ok(mf, g, {**MD, "album": 2})


def test_missing_field_rules(mf):
    md = {}
    for op, operand in [("$eq", 1), ("$gt", 1), ("$gte", 1), ("$lt", 1), ("$lte", 1), ("$in", [1])]:
        assert not ok(mf, {"x": {op: operand}}, md), op
    assert not ok(mf, {"x": 1}, md)
    assert ok(mf, {"x": {"$ne": 1}}, md)
    assert ok(mf, {"x": {"$nin": [1]}}, md)


def test_list_valued_fields(mf):
    assert ok(mf, {"tag": "cat"}, MD)
    assert ok(mf, {"tag": {"$eq": "pet"}}, MD)
    assert not ok(mf, {"tag": "dog"}, MD)
    assert ok(mf, {"tag": {"$in": ["dog", "pet"]}}, MD)
    assert not ok(mf, {"tag": {"$in": ["dog", "bird"]}}, MD)
    assert not ok(mf, {"tag": {"$ne": "cat"}}, MD)   # the negation of $eq
    assert ok(mf, {"tag": {"$ne": "dog"}}, MD)
    assert not ok(mf, {"tag": {"$nin": ["cat"]}}, MD)
    assert ok(mf, {"tag": {"$nin": ["dog"]}}, MD)
    assert not ok(mf, {"tag": {"$gt": 0}}, MD)        # a list is not a number


def test_number_and_bool_typing(mf):
    # $gt .. $lte: numbers with numbers only; bool is not a number
    assert not ok(mf, {"public": {"$gt": 0}}, MD)
    assert not ok(mf, {"public": {"$gte": 1}}, MD)
    assert not ok(mf, {"owner": {"$gt": 0}}, MD)
    assert not ok(mf, {"n": {"$lt": 1}}, {"n": False})
    assert ok(mf, {"n": {"$lt": 1}}, MD)
    # equality is typed the same way
    assert ok(mf, {"public": True}, MD)
    assert not ok(mf, {"public": 1}, MD)
    assert not ok(mf, {"n": False}, MD)
    assert ok(mf, {"n": 0.0}, MD)
    assert not ok(mf, {"album": "3"}, MD)
    assert ok(mf, {"public": {"$ne": 1}}, MD)
    assert not ok(mf, {"public": {"$in": [1, 0]}}, MD)
    assert ok(mf, {"public": {"$in": [False, True]}}, MD)


@pytest.mark.parametrize("bad", [
    {"album": {"$regex": "a"}},            # unknown field operator
    {"$not": [{"album": 1}]},              # unknown logical operator
    {"album": {"$in": 3}},                 # $in without a list
    {"album": {"$nin": "ab"}},
    {"album": {"$in": [[1]]}},
    {"$and": {"album": 1}},                # $and without a list
    {"$and": [1, 2]},                      # ... of dicts
    {"$or": []},
    {"$or": "x"},
    {"album": {"$gt": "3"}},               # range operand must be a number
    {"album": {"$lte": True}},
    {"album": {"$exists": 1}},
    {"album": {"$eq": [1, 2]}},
    {"album": {"$eq": None}},
    {"album": None},
    {"album": {}},
    {"$and": [{"album": {"$bogus": 1}}]},  # nested errors surface too
])
def test_malformed_filters_raise_value_error(mf, bad):
    with pytest.raises(ValueError):
        mf.compile_filter(bad)


def test_filter_must_be_a_dict(mf):
    for bad in ([], "album", 3, None):
        with pytest.raises(ValueError):
            mf.compile_filter(bad)


def test_canonical_json_is_key_order_independent(mf):
    assert mf.canonical({"a": 1, "b": {"$in": [1, 2]}}) == mf.canonical({"b": {"$in": [1, 2]}, "a": 1})
    assert mf.canonical({"a": 1}) != mf.canonical({"a": 2})
    with pytest.raises(ValueError):
        mf.canonical({"a": {1, 2}})


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000])
def test_bitmap_layout(mf, n):
    rng = np.random.default_rng(n)
    flags = rng.random(n) < 0.5
    flags[0] = True
    flags[n - 1] = True
    ids = [f"id{r}" for r in range(n)]
    meta = {i: {"keep": bool(f)} for i, f in zip(ids, flags)}
    del meta[ids[0]]  # a vector without metadata counts as {}
    flags[0] = False
    bm, count = mf.build_bitmap(mf.compile_filter({"keep": True}), ids, meta)
    assert bm.dtype == np.uint32 and bm.flags["C_CONTIGUOUS"]
    assert bm.shape == ((n + 31) // 32,)
    assert count == int(flags.sum())
    # bit r & 31 of word r >> 5 is row r; padding bits are clear
    for r in range(32 * bm.shape[0]):
        bit = (int(bm[r >> 5]) >> (r & 31)) & 1
        assert bit == (int(flags[r]) if r < n else 0), r
    # little-endian words: byte b of the buffer holds rows 8b .. 8b + 7
    raw = np.frombuffer(bm.tobytes(), dtype=np.uint8)
    for r in (0, n - 1):
        assert (int(raw[r >> 3]) >> (r & 7)) & 1 == int(flags[r])
    all_bm, all_count = mf.build_bitmap(mf.compile_filter({}), ids, meta)
    assert all_count == n and int(sum(bin(int(w)).count("1") for w in all_bm)) == n


def test_masked_sharded_calls_reject_a_null_handle_before_any_device_call():
    L = import_pkg("_lib")
    lib = L.load()
    st = lib.rc_sharded_search_masked(None, None, 1, 10, 5, None, None, None, L.RC_SEARCH_AUTO, None)
    assert st == L.RC_ERR_INVALID
    assert lib.rc_last_error()
    st = lib.rc_sharded_query_host_masked(None, None, 1, 10, 5, 0, None, None, None, None)
    assert st == L.RC_ERR_INVALID
    st = lib.rc_index_search_masked(None, None, 1, 10, 5, None, None, None, L.RC_SEARCH_AUTO, None)
    assert st == L.RC_ERR_INVALID
    h = ctypes.c_void_p()  # still NULL
    assert lib.rc_sharded_search_masked(h, None, 1, 10, 5, None, None, None, L.RC_SEARCH_AUTO, None) == L.RC_ERR_INVALID


def test_retriever_search_passes_filter_only_when_given():
    """A reference-shaped index object whose ``query`` knows nothing of filters keeps working."""
    utils = import_pkg("retriever.utils")

    class Plain:
        def query(self, vector, top_k, include_values):
            return {"matches": [{"id": "a"}, {"id": "b"}]}

    class Filtering:
        def query(self, vector, top_k, include_values, filter=None):
            self.seen = filter
            return {"matches": [{"id": "c"}]}

    assert utils.search(Plain(), [0.1, 0.2], 2) == ["a", "b"]
    assert utils.search(Plain(), [0.1, 0.2], 2, filter=None) == ["a", "b"]
    f = Filtering()
    assert utils.search(f, [0.1], 1, filter={"x": 1}) == ["c"] and f.seen == {"x": 1}
    with pytest.raises(ValueError):
        utils.search(Plain(), [], 2, filter={"x": 1})
