"""Metadata columns, host side (``metacolumns``): the value encoder, the filter compiler, the
numpy model of ``rc_meta_eval`` (``run_program``) against ``metafilter`` itself, the page-list
addressing, ``Index(metadata_config=...)``'s validation and the library entries' argument checks,
which all run before any device call (so on a host without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

import metacolumns_corpus as corpus
from conftest import REPO, import_pkg


@pytest.fixture(scope="module")
def mc():
    return import_pkg("metacolumns")


@pytest.fixture(scope="module")
def mf():
    return import_pkg("metafilter")


def bits(x):
    return np.array([x], dtype=np.float64).view(np.int64)[0].item()


# ------------------------------------------------------------------ encoder --
def test_encoder_type_rules(mc):
    codes = {}
    assert mc.encode_value(True, codes) == (mc.TAG_BOOL, 1) and mc.encode_value(False, codes) == (mc.TAG_BOOL, 0)
    assert mc.encode_value(1, codes) == (mc.TAG_NUMBER, bits(1.0))           # True is not 1 ...
    assert mc.encode_value(1, codes) == mc.encode_value(1.0, codes)          # ... and 1 is 1.0
    assert mc.encode_value(2 ** 53, codes) == (mc.TAG_NUMBER, bits(float(2 ** 53)))
    assert mc.encode_value(2 ** 53 + 1, codes) is None                       # float64 cannot hold it
    assert mc.encode_value(10 ** 400, codes) is None                         # nor this (float() overflows)
    assert mc.encode_value(-0.0, codes) == (mc.TAG_NUMBER, bits(-0.0)) != mc.encode_value(0.0, codes)
    tag, val = mc.encode_value(float("nan"), codes)
    assert tag == mc.TAG_NUMBER and np.isnan(np.array([val], dtype=np.int64).view(np.float64)[0])
    assert mc.encode_value("red", codes) == (mc.TAG_STRING, 0) and mc.encode_value("blue", codes) == (mc.TAG_STRING, 1)
    assert mc.encode_value("red", codes) == (mc.TAG_STRING, 0) and codes == {"red": 0, "blue": 1}
    assert mc.encode_value("green", codes, add=False) == (mc.TAG_STRING, -1) and "green" not in codes

    class MyStr(str):
        pass

    class MyInt(int):
        pass

    for bad in ([1, 2], ("a",), None, {"a": 1}, MyStr("red"), MyInt(3), np.float64(1.5), np.int64(3), np.bool_(True),
                np.float32(2.0), b"red"):
        assert mc.encode_value(bad, codes) is None, type(bad)


def test_field_index_encodes_rows_and_demotes(mc):
    fx = mc.FieldIndex(["a", "b", "c"])
    tags, vals = fx.encode([{"a": 1, "b": "x"}, {"b": "y", "c": True, "other": [1]}, {}])
    assert tags.dtype == np.uint8 and vals.dtype == np.int64 and tags.shape == vals.shape == (3, 3)
    assert tags.tolist() == [[1, 0, 0], [3, 3, 0], [0, 2, 0]]
    assert vals[0, 0] == bits(1.0) and vals[1].tolist()[:2] == [0, 1] and vals[2, 1] == 1
    assert fx.demoted == {} and fx.stats()["device"] == ["a", "b", "c"]
    # a list demotes its field, and only it; the reason names the type; nothing re-promotes it
    tags, _ = fx.encode([{"a": 2, "b": ["x", "y"]}, {"a": np.float64(2.0), "c": False}])
    assert set(fx.demoted) == {"b", "a"} and "list" in fx.demoted["b"] and "float64" in fx.demoted["a"]
    assert tags[1].tolist() == [0, 0] and tags[2].tolist() == [0, 2]
    fx.encode([{"a": 1, "b": "x"}])
    st = fx.stats()
    assert st["device"] == ["c"] and st["indexed"] == ["a", "b", "c"] and st["valid"] is True
    assert fx.program({"c": True}) is not None and fx.program({"a": 1}) is None and fx.program({"b": "x", "c": True}) is None


# ------------------------------------------------------------------- parity --
@pytest.fixture(scope="module")
def world(mc):
    metas = corpus.gen_metas(500, seed=11)
    filters = corpus.gen_filters(300, seed=12)
    fx, tags, vals = corpus.encode_all(mc, metas)
    return metas, filters, fx, tags, vals


def test_the_corpus_covers_the_language(world):
    metas, filters, fx, tags, vals = world
    used = set()
    for f in filters:
        corpus.ops_used(f, used)
    assert used >= set(corpus.OPS) | {"$and", "$or", "bare"}
    assert max(corpus.depth_of(f) for f in filters) == 4  # a field dict under three levels of $and / $or
    flat = repr(filters)
    assert "'$in': []" in flat and "'$nin': []" in flat and corpus.UNKNOWN[0] in flat
    absent = 1.0 - sum(len(m) for m in metas) / (len(metas) * len(corpus.FIELDS))
    assert 0.25 < absent < 0.35
    assert {int(t) for t in np.unique(tags)} == {0, 1, 2, 3}


def test_run_program_equals_the_host_predicate_on_every_corpus_filter(world, mc, mf):
    metas, filters, fx, tags, vals = world
    n = len(metas)
    nonempty = 0
    for flt in filters:
        prog = fx.program(flt)
        assert prog is not None, flt  # every corpus filter has a program
        pred = mf.compile_filter(flt)
        flags = np.array([bool(pred(m)) for m in metas])
        words, count = mc.run_program(prog, tags, vals, n)
        assert words.dtype == np.uint32 and words.shape == ((n + 31) // 32,)
        assert np.array_equal(words, mf.pack_bits(flags)), flt
        assert count == int(flags.sum())
        nonempty += 0 < count < n
    assert nonempty > 100  # the corpus is not made of trivial filters


def test_run_program_is_build_bitmap_bit_for_bit(world, mc, mf):
    metas, filters, fx, tags, vals = world
    ids = [f"id{i}" for i in range(len(metas))]
    meta = {i: m for i, m in zip(ids, metas) if m}  # a vector without metadata has no entry
    for n in (0, 1, 31, 32, 33, 500):
        for flt in filters[:40]:
            want = mf.build_bitmap(mf.compile_filter(flt), ids[:n], meta)
            got = mc.run_program(fx.program(flt), tags, vals, n)
            assert got[0].dtype == want[0].dtype and np.array_equal(got[0], want[0]) and got[1] == want[1]


def test_ieee_and_typed_comparisons(mc, mf):
    metas = [{"x": -0.0}, {"x": 0.0}, {"x": 0}, {"x": float("nan")}, {"x": True}, {"x": 1}, {"x": "1"}, {}, {"x": False}]
    fx, tags, vals = corpus.encode_all(mc, metas, fields=["x"])
    nan = float("nan")
    for flt in ({"x": 0.0}, {"x": -0.0}, {"x": {"$ne": 0}}, {"x": nan}, {"x": {"$ne": nan}}, {"x": {"$in": [nan, 1]}},
                {"x": {"$gte": nan}}, {"x": {"$lt": nan}}, {"x": True}, {"x": 1}, {"x": {"$ne": True}}, {"x": "1"},
                {"x": {"$gt": 0}}, {"x": {"$gte": 0}}, {"x": {"$lte": 1.0}}, {"x": {"$lt": 1}}, {"x": {"$nin": [False, "1"]}},
                {"x": {"$exists": False}}, {"x": {"$exists": True}}, {"x": {"$gt": -1e308, "$lt": 1e308}}):
        pred = mf.compile_filter(flt)
        want = mf.pack_bits([pred(m) for m in metas])
        words, _ = mc.run_program(fx.program(flt), tags, vals, len(metas))
        assert np.array_equal(words, want), flt


# ----------------------------------------------------------------- compiler --
def test_program_shape_and_field_ordering(mc):
    fields = ["a", "b", "c"]
    dicts = {"a": {"x": 0}, "b": {}, "c": {}}
    prog = mc.compile_program({"b": 1, "a": {"$in": ["x", "nope"]}, "c": {"$exists": True}, "$or": [{"b": 2}, {"a": "x"}]},
                              fields, dicts)
    assert prog.dtype == np.int64 and prog.shape[1] == 2
    mc.check_program(prog, 3)
    ops = (prog[:, 0] & 0xFF).tolist()
    assert ops.count(mc.OP_EQ) == 5 and ops.count(mc.OP_EXISTS) == 1 and set(ops) <= {mc.OP_EQ, mc.OP_EXISTS, mc.OP_AND, mc.OP_OR}
    assert all((w >> 32) == 2 for w in prog[:, 0].tolist() if (w & 0xFF) in (mc.OP_AND, mc.OP_OR))
    # the top-level AND's own leaves come first, grouped by field: b, then c; then the nested groups
    leaf_fields = [(w >> 8) & 0xFF for w in prog[:, 0].tolist() if (w & 0xFF) <= mc.OP_NOT_EXISTS]
    assert leaf_fields[:2] == [1, 2]
    # a string the dictionary does not hold is code -1; a known one its code; the dictionary is not written
    eq_a = [(int(w), int(v)) for w, v in prog.tolist() if (w & 0xFF) == mc.OP_EQ and (w >> 8) & 0xFF == 0]
    assert sorted(v for _, v in eq_a) == [-1, 0, 0] and dicts["a"] == {"x": 0}
    assert mc.compile_program({"a": {"$in": []}}, fields, dicts)[:, 0].tolist() == [mc.OP_FALSE]
    assert mc.compile_program({"a": {"$nin": []}}, fields, dicts)[:, 0].tolist() == [mc.OP_TRUE]


def test_compile_program_returns_none_where_the_host_must_evaluate(mc):
    fields, dicts = ["a", "b"], {"a": {}, "b": {}}

    class MyInt(int):
        pass

    assert mc.compile_program({"a": 1}, fields, dicts) is not None
    assert mc.compile_program({"zzz": 1}, fields, dicts) is None                       # not indexed
    assert mc.compile_program({"$or": [{"a": 1}, {"zzz": 1}]}, fields, dicts) is None
    assert mc.compile_program({"a": 1, "b": 2}, fields, dicts, demoted={"b": "a list"}) is None  # demoted
    assert mc.compile_program({"a": 1}, fields, dicts, demoted={"b": "a list"}) is not None
    assert mc.compile_program({"a": 2 ** 53 + 1}, fields, dicts) is None               # unencodable operands
    assert mc.compile_program({"a": {"$gt": 10 ** 400}}, fields, dicts) is None
    assert mc.compile_program({"a": {"$in": [1, MyInt(2)]}}, fields, dicts) is None
    assert mc.compile_program({"a": np.float64(1.0)}, fields, dicts) is None
    # the limits: 64 leaves and 16 levels are inside them, an $in past MAX_INSTR / 2 leaves is not
    assert mc.compile_program({"a": {"$in": list(range(64))}}, fields, dicts).shape[0] == 127
    assert mc.compile_program({"a": {"$in": list(range(256))}}, fields, dicts).shape[0] == 511 <= mc.MAX_INSTR
    assert mc.compile_program({"a": {"$in": list(range(257))}}, fields, dicts) is None
    deep = {"a": 1, "b": {"$in": [1, 2]}}
    for _ in range(16):
        deep = {"a": 1, "$or": [{"b": 2}, deep]}
    prog = mc.compile_program(deep, fields, dicts)
    assert prog is not None
    mc.check_program(prog, 2)
    for _ in range(40):
        deep = {"a": 1, "$or": [{"b": 2}, deep]}
    assert mc.compile_program(deep, fields, dicts) is None                             # past MAX_STACK


@pytest.mark.parametrize("bad", [{"a": {"$foo": 1}}, {"a": {"$in": 3}}, {"$and": []}, {"$and": [1]}, {"a": {"$gt": "x"}},
                                 {"a": {"$exists": 1}}, {"$nor": [{"a": 1}]}, {"a": {}}, {"a": [1, 2]}, {"a": None}, [("a", 1)],
                                 {"zzz": {"$gt": True}}, {1: 2}])
def test_malformed_filters_raise_what_compile_filter_raises(mc, mf, bad):
    with pytest.raises(ValueError) as want:
        mf.compile_filter(bad)
    with pytest.raises(ValueError) as got:
        mc.compile_program(bad, ["a"], {"a": {}})
    assert str(got.value) == str(want.value)


def test_check_program_refuses_what_the_kernel_must_never_run(mc):
    leaf = lambda f=0, op=0, tag=1: op | f << 8 | tag << 16  # noqa: E731
    comb = lambda op, k: op | k << 32                        # noqa: E731
    ok = np.array([[leaf(), 0], [leaf(1), 0], [comb(mc.OP_AND, 2), 0]], dtype=np.int64)
    mc.check_program(ok, 2)
    for bad in ([[leaf(2), 0]],                                   # field past n_fields
                [[leaf(), 0], [comb(mc.OP_AND, 2), 0]],           # underflow
                [[leaf(), 0], [leaf(), 0]],                       # two results left
                [[comb(mc.OP_OR, 0), 0]], [[12, 0]], [[leaf(tag=0), 0]], [[leaf(tag=4), 0]], [[-1, 0]],
                [[mc.OP_TRUE, 0]] * (mc.MAX_STACK + 1) + [[comb(mc.OP_AND, mc.MAX_STACK + 1), 0]],
                [[mc.OP_TRUE, 0]] + [[comb(mc.OP_AND, 1), 0]] * mc.MAX_INSTR):
        with pytest.raises(ValueError):
            mc.check_program(np.array(bad, dtype=np.int64).reshape(-1, 2), 2)
    with pytest.raises(ValueError):
        mc.check_program(np.zeros((0, 2), dtype=np.int64), 2)


# ------------------------------------------------------------ page addressing --
@pytest.mark.parametrize("shards", [1, 2])
def test_run_program_page_addressing_is_positions_to_rows(mc, mf, shards):
    pages = import_pkg("pages")
    span = pages.span(shards)
    page_list = [5, 0, 3]
    n = 2 * span + 77
    metas = corpus.gen_metas(n, seed=5)
    rows = pages.positions_to_rows(page_list, range(n), shards)
    cap = 6 * span
    fx = mc.FieldIndex(corpus.FIELDS)
    t, v = fx.encode(metas)
    tags, vals = np.full((5, cap), mc.TAG_BOOL, dtype=np.uint8), np.ones((5, cap), dtype=np.int64)  # decoys elsewhere
    tags[:, rows], vals[:, rows] = t, v
    for flt in corpus.gen_filters(25, seed=6):
        pred = mf.compile_filter(flt)
        want = mf.pack_bits([pred(m) for m in metas])
        words, count = mc.run_program(fx.program(flt), tags, vals, n, pages=page_list, span=span)
        assert np.array_equal(words, want) and count == int(np.unpackbits(want.view(np.uint8)).sum())
    with pytest.raises(ValueError):
        mc.run_program(fx.program({"flag": True}), tags, vals, 3 * span + 1, pages=page_list, span=span)
    with pytest.raises(ValueError):
        mc.run_program(fx.program({"flag": True}), tags, vals, n, pages=[5, 0, 6], span=span)


# ------------------------------------------------------------------ the config --
@pytest.mark.parametrize("cfg", [[], "color", {"indexed": "color"}, {"indexed": ["a"], "extra": 1}, {}, {"fields": ["a"]},
                                 {"indexed": ["a", "a"]}, {"indexed": ["a", ""]}, {"indexed": ["a", 3]}, {"indexed": ("a",)},
                                 {"indexed": ["$a"]}, {"indexed": [f"f{i}" for i in range(65)]}])
def test_metadata_config_is_validated_before_any_device_work(mc, monkeypatch, cfg):
    idx = import_pkg("index")

    def no_device(*a, **k):
        raise AssertionError("the constructor reached the device")

    monkeypatch.setattr(idx, "ShardSet", no_device)
    with pytest.raises(ValueError, match="metadata_config"):
        idx.Index("bad", dimension=64, metadata_config=cfg)
    with pytest.raises(ValueError):
        mc.validate_config(cfg)


def test_accepted_configs_and_the_default(mc, monkeypatch):
    assert mc.validate_config(None) is None
    assert mc.validate_config({"indexed": ["a", "b c", "ü"]}) == ["a", "b c", "ü"]
    assert mc.validate_config({"indexed": []}) == []
    assert mc.DEVICE_MIN_ROWS >= 0
    idx = import_pkg("index")

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()

    monkeypatch.setattr(idx, "ShardSet", stop)
    for cfg in (None, {"indexed": ["a"]}, {"indexed": []}):
        with pytest.raises(Reached):
            idx.Index("ok", dimension=64, metadata_config=cfg)


def test_the_configured_field_list_reaches_get_index(monkeypatch):
    cfgmod = import_pkg("config")
    assert cfgmod.comma_list("") == [] and cfgmod.comma_list(" color, size ,,flag") == ["color", "size", "flag"]
    assert cfgmod.Config.INDEX_METADATA_FIELDS == cfgmod.comma_list(os.environ.get("RC_INDEX_METADATA_FIELDS", ""))
    utils, idx = import_pkg("ingesting.utils"), import_pkg("index")
    made = []

    class FakeIndex:
        def __init__(self, name, **kw):
            made.append(kw)

    monkeypatch.setattr(idx, "Index", FakeIndex)
    monkeypatch.setattr(utils, "_indexes", {})
    monkeypatch.setattr(utils.Config, "INDEX_METADATA_FIELDS", [])
    utils.get_index("plain", devices=[0])
    monkeypatch.setattr(utils.Config, "INDEX_METADATA_FIELDS", ["color", "size"])
    utils.get_index("columns", devices=[0])
    assert made[0]["metadata_config"] is None and made[1]["metadata_config"] == {"indexed": ["color", "size"]}


# --------------------------------------------------------------------- the ABI --
def test_header_and_module_constants_agree(mc):
    text = open(os.path.join(REPO, "include", "retrieval_core.h")).read()
    assert "Metadata columns" in text
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+RC_META_(\w+)\s+(\d+)", text, flags=re.M)}
    for name in ("EQ", "NE", "GT", "GE", "LT", "LE", "EXISTS", "NOT_EXISTS", "TRUE", "FALSE", "AND", "OR"):
        assert defs[name] == getattr(mc, "OP_" + name)
    for name in ("ABSENT", "NUMBER", "BOOL", "STRING"):
        assert defs["TAG_" + name] == getattr(mc, "TAG_" + name)
    assert (defs["MAX_FIELDS"], defs["MAX_INSTR"], defs["MAX_STACK"]) == (mc.MAX_FIELDS, mc.MAX_INSTR, mc.MAX_STACK)
    assert mc.MAX_INSTR >= 2 * 64 - 1 and mc.MAX_STACK >= 2 * 16 + 3  # 64 leaves, 16 levels
    L = import_pkg("_lib")
    assert L.load().rc_abi_version() == 1
    for fn in ("rc_meta_write", "rc_meta_move", "rc_meta_eval"):
        assert fn in L.SIGNATURES and re.search(r"^int " + fn + r"\(", text, flags=re.M)


def test_entries_refuse_bad_arguments_before_any_device_call(mc):
    """RC_ERR_INVALID on a host without a GPU: no pointer is dereferenced on the device and no
    HIP call is made before the checks pass."""
    L = import_pkg("_lib")
    lib = L.load()
    buf = (ctypes.c_uint64 * 64)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15  # never read: the checks come first
    leaf = lambda f=0: mc.OP_EQ | f << 8 | mc.TAG_NUMBER << 16  # noqa: E731

    def ev(prog, n_fields=2, cap=1024, n=100, pages=None, span=0, tags=p, vals=p, ws=p, ws_bytes=512, words=p, count=p):
        prog = np.ascontiguousarray(prog, dtype=np.int64).reshape(-1, 2)
        pg = None if pages is None else np.ascontiguousarray(pages, dtype=np.int32)
        st = lib.rc_meta_eval(tags, vals, n_fields, cap, prog.ctypes.data if prog.size else None, prog.shape[0],
                              None if pg is None else pg.ctypes.data, 0 if pg is None else len(pg), span, n, ws, ws_bytes,
                              words, count, None)
        return st, lib.rc_last_error()

    good = [[leaf(), 0], [leaf(1), 0], [mc.OP_OR | 2 << 32, 0]]
    for kw, what in (({"tags": None}, b"null"), ({"vals": None}, b"null"), ({"words": None}, b"null"), ({"count": None}, b"null"),
                     ({"ws": None}, b"workspace"), ({"ws": p + 8}, b"aligned"), ({"ws_bytes": 47}, b"workspace"),
                     ({"n_fields": 0}, b"n_fields"), ({"n_fields": 65}, b"n_fields"), ({"cap": 0}, b"capacity"),
                     ({"n": 1025}, b"capacity"), ({"n": -1}, b"n must"), ({"n_fields": 1}, b"field"),
                     ({"pages": [0, 1], "span": 100}, b"span"), ({"pages": [0, 2], "span": 512}, b"page at or past"),
                     ({"pages": [0, 4], "span": 256}, b"page at or past"), ({"pages": [0, -1], "span": 256}, b"page at or past"),
                     ({"pages": [0], "span": 256, "n": 257}, b"beyond the page list"),
                     ({"pages": [0, 1], "span": 256, "ws_bytes": 55}, b"workspace")):
        st, msg = ev(good, **kw)
        assert st == L.RC_ERR_INVALID and what in msg, (kw, msg)
    for prog, what in (([[leaf(), 0], [mc.OP_AND | 2 << 32, 0]], b"underflows"), ([[leaf(), 0], [leaf(), 0]], b"exactly one"),
                       ([[12, 0]], b"unknown"), ([[mc.OP_EQ, 0]], b"operand tag"), ([], b"program"),
                       ([[mc.OP_TRUE, 0]] * 65 + [[mc.OP_AND | 65 << 32, 0]], b"MAX_STACK")):
        st, msg = ev(prog, ws_bytes=1 << 20)
        assert st == L.RC_ERR_INVALID and what in msg, (prog[:2], msg)
    # the same programs are refused by the Python twin of the check
    for prog in ([[leaf(), 0], [mc.OP_AND | 2 << 32, 0]], [[12, 0]]):
        with pytest.raises(ValueError):
            mc.check_program(np.array(prog, dtype=np.int64), 2)
    for fn, args in ((lib.rc_meta_write, (None, p, 2, 100, p, p, p, 1, None)), (lib.rc_meta_write, (p, p, 0, 100, p, p, p, 1, None)),
                     (lib.rc_meta_write, (p, p, 2, 100, None, p, p, 1, None)), (lib.rc_meta_write, (p, p, 2, 100, p, p, p, 101, None)),
                     (lib.rc_meta_write, (p, p, 2, 100, p, p, p, -1, None)), (lib.rc_meta_move, (p, None, 2, 100, p, p, 1, None)),
                     (lib.rc_meta_move, (p, p, 2, 100, p, None, 1, None)), (lib.rc_meta_move, (p, p, 2, 0, p, p, 1, None)),
                     (lib.rc_meta_move, (p, p, 2, 100, p, p, 101, None))):
        assert fn(*args) == L.RC_ERR_INVALID
    assert lib.rc_meta_write(p, p, 2, 100, None, None, None, 0, None) == L.RC_OK  # nothing to do: no device call either
    assert lib.rc_meta_move(p, p, 2, 100, None, None, 0, None) == L.RC_OK
