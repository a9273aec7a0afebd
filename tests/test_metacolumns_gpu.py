"""Metadata columns on the GPU: ``rc_meta_write`` / ``rc_meta_move`` / ``rc_meta_eval`` against the
numpy model (``metacolumns.run_program``, itself held to ``metafilter`` by the CPU tests), and
``Index(metadata_config=...)`` against an index without it: equal answers on every path, with
``metadata_index_stats`` proving which path built each bitmap."""
import json
import os
import random

import numpy as np
import pytest

import metacolumns_corpus as corpus
from conftest import import_pkg

pytestmark = pytest.mark.gpu

DIM = 64
SIZES = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 5077]
DECOYS = 300


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


@pytest.fixture(scope="module")
def mc(cuda):
    return import_pkg("metacolumns")


@pytest.fixture(scope="module")
def mf():
    return import_pkg("metafilter")


@pytest.fixture(autouse=True)
def device_path_at_every_size(mc, monkeypatch):
    monkeypatch.setattr(mc, "DEVICE_MIN_ROWS", 0)


# ------------------------------------------------------------------ the kernels --
@pytest.fixture(scope="module")
def world(mc, mf):
    """5077 corpus rows, one decoy row, and a dozen corpus filters the decoy satisfies (so a row
    read past n would set a bit and raise the count), encoded once with one dictionary."""
    metas = corpus.gen_metas(max(SIZES), seed=21)
    decoy = {"color": "red", "size": 3, "flag": True, "score": 2.5}
    preds = [(f, mf.compile_filter(f)) for f in corpus.gen_filters(300, seed=22)]
    chosen = [f for f, p in preds if p(decoy) and 0 < sum(map(p, metas[:257])) < 257][:12]
    assert len(chosen) == 12
    fx = mc.FieldIndex(corpus.FIELDS)
    tags, vals = fx.encode(metas + [decoy])
    assert fx.demoted == {}
    programs = [fx.program(f) for f in chosen]
    assert all(p is not None for p in programs)
    return metas, tags, vals, programs


def columns_with_decoys(world, n):
    metas, tags, vals, _ = world
    last = tags.shape[1] - 1
    t = np.concatenate([tags[:, :n], np.repeat(tags[:, last:], DECOYS, axis=1)], axis=1)
    v = np.concatenate([vals[:, :n], np.repeat(vals[:, last:], DECOYS, axis=1)], axis=1)
    return np.ascontiguousarray(t), np.ascontiguousarray(v)


@pytest.fixture(scope="module")
def device_columns(mc, cuda):
    return mc.Columns(len(corpus.FIELDS), max(SIZES) + DECOYS + 11, cuda)


@pytest.mark.parametrize("n", SIZES)
def test_eval_equals_the_model_words_and_count(world, device_columns, mc, n):
    t, v = columns_with_decoys(world, n)
    device_columns.write(list(range(n + DECOYS)), t, v)  # (rc_meta_write: every field of every row)
    for prog in world[3]:
        want_words, want_count = mc.run_program(prog, t, v, n)
        _, with_decoys = mc.run_program(prog, t, v, n + DECOYS)
        assert with_decoys == want_count + DECOYS  # the rows past n do satisfy the filter
        words, count = device_columns.eval(prog, n)
        assert words.dtype == np.uint32 and words.shape == ((n + 31) // 32,)
        assert np.array_equal(words, want_words) and count == want_count


def test_eval_of_nothing_and_of_hand_written_combinators(world, device_columns, mc):
    n = 257
    t, v = columns_with_decoys(world, n)
    device_columns.write(list(range(n + DECOYS)), t, v)
    words, count = device_columns.eval(world[3][0], 0)
    assert words.shape == (0,) and count == 0
    leaf = lambda op, f, tag=mc.TAG_NUMBER, val=0: [op | f << 8 | tag << 16, val]  # noqa: E731
    three = mc.float_bits(3.0)
    progs = [
        # AND(3) / OR(3) / AND(1): the n-ary forms the compiler never emits
        [leaf(mc.OP_EXISTS, 0), leaf(mc.OP_GE, 1, val=three), leaf(mc.OP_NE, 2, mc.TAG_BOOL, 1), [mc.OP_AND | 3 << 32, 0]],
        [leaf(mc.OP_NOT_EXISTS, 4), leaf(mc.OP_LT, 3, val=three), leaf(mc.OP_EQ, 2, mc.TAG_BOOL, 0), [mc.OP_OR | 3 << 32, 0]],
        [leaf(mc.OP_LE, 1, val=three), [mc.OP_AND | 1 << 32, 0], [mc.OP_TRUE, 0], [mc.OP_FALSE, 0], [mc.OP_OR | 2 << 32, 0],
         [mc.OP_AND | 2 << 32, 0]],
        [[mc.OP_TRUE, 0]] * 64 + [[mc.OP_AND | 64 << 32, 0]],  # the whole 64-entry stack
        [[mc.OP_FALSE, 0]] * 63 + [leaf(mc.OP_GT, 1, val=three), [mc.OP_OR | 64 << 32, 0]],
    ]
    for p in progs:
        prog = np.array(p, dtype=np.int64)
        want_words, want_count = mc.run_program(prog, t, v, n)
        words, count = device_columns.eval(prog, n)
        assert np.array_equal(words, want_words) and count == want_count
    assert device_columns.eval(np.array(progs[3], dtype=np.int64), n)[1] == n


@pytest.mark.parametrize("span", [256, 512])
def test_eval_through_a_shuffled_page_list(world, mc, cuda, span):
    metas, tags, vals, programs = world
    n = max(SIZES)
    n_pages = -(-n // span)
    page_list = list(range(n_pages + 3))
    random.Random(span).shuffle(page_list)
    page_list = page_list[:n_pages]
    assert page_list != sorted(page_list)
    cap = (n_pages + 3) * span
    last = tags.shape[1] - 1
    pos = np.arange(n)
    rows = np.asarray(page_list)[pos // span] * span + pos % span
    t = np.ascontiguousarray(np.repeat(tags[:, last:], cap, axis=1))  # decoys in every row no position maps to
    v = np.ascontiguousarray(np.repeat(vals[:, last:], cap, axis=1))
    t[:, rows], v[:, rows] = tags[:, :n], vals[:, :n]
    cols = mc.Columns(len(corpus.FIELDS), cap, cuda)
    cols.write(list(range(cap)), t, v)
    for m in (n, span, span + 1, 33):
        for prog in programs:
            want_words, want_count = mc.run_program(prog, t, v, m, pages=page_list, span=span)
            dense = mc.run_program(prog, tags, vals, m)
            assert np.array_equal(want_words, dense[0]) and want_count == dense[1]
            words, count = cols.eval(prog, m, pages=page_list, span=span)
            assert np.array_equal(words, want_words) and count == want_count


def test_move_copies_every_field_and_write_reaches_only_its_rows(world, mc, cuda):
    metas, tags, vals, programs = world
    n = 1000
    t, v = np.ascontiguousarray(tags[:, :n]), np.ascontiguousarray(vals[:, :n])
    cols = mc.Columns(len(corpus.FIELDS), n, cuda)
    cols.write(list(range(n)), t, v)
    rng = np.random.default_rng(3)
    perm = rng.permutation(n)
    src, dst = perm[:300], perm[300:600]
    cols.move(src.tolist(), dst.tolist())
    t[:, dst], v[:, dst] = t[:, src], v[:, src]
    rows = perm[600:700]
    t[:, rows], v[:, rows] = tags[:, 2000:2100], vals[:, 2000:2100]
    cols.write(rows.tolist(), np.ascontiguousarray(t[:, rows]), np.ascontiguousarray(v[:, rows]))
    assert np.array_equal(cols.tags.cpu().numpy(), t) and np.array_equal(cols.vals.cpu().numpy(), v)
    for prog in programs:
        want = mc.run_program(prog, t, v, n)
        got = cols.eval(prog, n)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    cols.ensure(4 * n)  # growing keeps what is stored
    assert cols.capacity == 4 * n and np.array_equal(cols.tags[:, :n].cpu().numpy(), t)
    got = cols.eval(programs[0], n)
    want = mc.run_program(programs[0], t, v, n)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    with pytest.raises(ValueError):
        cols.write([4 * n], t[:, :1], v[:, :1])
    with pytest.raises(ValueError):
        cols.eval(programs[0], 4 * n + 1)


# -------------------------------------------------------------------- the Index --
_VECS = {}


def vectors(n, seed):
    if (n, seed) not in _VECS:
        _VECS[(n, seed)] = np.random.default_rng(seed).standard_normal((n, DIM)).astype(np.float32)
    return _VECS[(n, seed)]


def index_filters(mf, metas, count=12, seed=32):
    """Distinct corpus filters (strict JSON) that some, not all, of ``metas`` satisfy."""
    out, seen = [], set()
    for f in corpus.gen_filters(400, seed=seed, special=False):
        p = mf.compile_filter(f)
        c = mf.canonical(f)
        if c not in seen and 0 < sum(map(p, metas)) < len(metas):
            seen.add(c)
            out.append(f)
        if len(out) == count:
            return out
    raise AssertionError("the corpus is too small")


def split_off_delete_filter(mf, filters, metas):
    """(the other filters, the one nearest to a quarter of ``metas``): ``delete(filter=)`` gets a filter
    no query used, and leaves most of the vectors."""
    pick = min(filters, key=lambda f: abs(sum(map(mf.compile_filter(f), metas)) - len(metas) // 4))
    return [f for f in filters if f is not pick], pick


class Pair:
    """The same operations on an index with ``metadata_config`` and on one without.  ``seen`` holds
    the distinct (filter, namespace, generation) triples the first one was asked for: its cache
    misses, as long as no filter comes back within one generation (the cache holds 8)."""

    def __init__(self, idxmod, cuda, shards, fields=corpus.FIELDS, name="pair"):
        kw = dict(dimension=DIM, capacity=256, devices=[cuda] * shards)
        self.dev = idxmod.Index(name, metadata_config={"indexed": list(fields)}, **kw)
        self.plain = idxmod.Index(name, **kw)
        self.gen = {}
        self.seen = set()
        self.nonempty = 0
        self.mf = import_pkg("metafilter")

    def each(self, fn, namespace=""):
        """A mutation of one namespace, on both indexes."""
        self.gen[namespace] = self.gen.get(namespace, 0) + 1
        a, b = fn(self.dev), fn(self.plain)
        assert a == b
        return a

    def upsert(self, ids, X, metas, namespace=""):
        import torch

        self.each(lambda ix: ix.upsert_tensor(ids, torch.from_numpy(X).cuda(), metas, namespace=namespace), namespace)

    def note(self, flt, namespace):
        key = (self.mf.canonical(flt), namespace, self.gen.get(namespace, 0))
        assert key not in self.seen, "the test repeats a filter within a generation: the miss count would be a guess"
        self.seen.add(key)

    def compare(self, filters, Q, namespace=""):
        for flt in filters:
            self.note(flt, namespace)
            got = [ix.query(vector=Q[0].tolist(), top_k=10, filter=flt, include_metadata=True, namespace=namespace)
                   for ix in (self.dev, self.plain)]
            assert got[0] == got[1], flt
            self.nonempty += bool(got[0]["matches"])
            for mode in ("auto", "scan"):
                got = [ix.query_batch(Q, top_k=7, filter=flt, mode=mode, namespace=namespace) for ix in (self.dev, self.plain)]
                assert got[0] == got[1], flt

    def delete_by_filter(self, flt, namespace=""):
        """``delete(filter=)`` on both; returns how many vectors it removed (equal on both)."""
        self.note(flt, namespace)
        counts = self.each(lambda ix: ix._delete(None, False, flt, namespace), namespace)
        assert self.dev.describe_index_stats() == self.plain.describe_index_stats()
        return counts

    def check_paths(self, host=0):
        st = self.dev.metadata_index_stats()
        assert st["valid"] is True
        assert st["device_evals"] + st["host_evals"] == len(self.seen)
        assert st["host_evals"] == host
        assert self.plain.metadata_index_stats()["device_evals"] == 0
        return st


@pytest.mark.parametrize("shards", [1, 2])
def test_index_with_columns_answers_as_the_index_without(idxmod, mf, cuda, shards):
    n = 700
    X, Q = vectors(n, 41), vectors(4, 42)
    metas = corpus.gen_metas(n, seed=43, special=False)
    ids = [f"v{i}" for i in range(n)]
    pair = Pair(idxmod, cuda, shards)
    filters, del_filter = split_off_delete_filter(mf, index_filters(mf, metas, count=13), metas)
    # 1. the initial upserts (two calls: the second grows the capacity and the columns with it)
    pair.upsert(ids[:200], X[:200], metas[:200])
    pair.upsert(ids[200:], X[200:], metas[200:])
    assert pair.dev._cols.capacity == pair.dev.capacity >= n
    pair.compare(filters, Q)
    pair.check_paths()
    assert pair.nonempty == len(filters)
    # 2. overwrites that change fields and drop them (every third loses all its metadata)
    new = corpus.gen_metas(150, seed=44, special=False)
    new = [{} if i % 3 == 0 else m for i, m in enumerate(new)]
    over = list(range(0, 600, 4))
    pair.upsert([ids[i] for i in over], X[over], new)
    for i, m in zip(over, new):
        metas[i] = m
    pair.compare(filters, Q)
    # 3. deletes that force compaction moves (rows from the front, survivors move down from the tail)
    gone = {ids[i] for i in range(5, 400, 3)}
    pair.each(lambda ix: ix.delete(ids=sorted(gone)))
    pair.compare(filters, Q)
    removed = pair.delete_by_filter(del_filter)
    live = [m for i, m in enumerate(metas) if ids[i] not in gone]
    assert removed == sum(map(mf.compile_filter(del_filter), live)) > 0
    pair.compare(filters, Q)
    # ... and the freed rows are reused by new ids with other metadata
    pair.upsert([f"w{i}" for i in range(120)], vectors(120, 45), corpus.gen_metas(120, seed=46, special=False))
    pair.compare(filters, Q)
    # 4. a named namespace on a shuffled page list, whose pool rows belonged to another namespace
    span = 256 * shards
    m = span + 44
    A, B = vectors(m, 47), vectors(m + span, 48)
    mb = corpus.gen_metas(m + span, seed=49, special=False)
    ib = [f"b{i}" for i in range(m + span)]
    pair.upsert([f"a{i}" for i in range(m)], A, corpus.gen_metas(m, seed=50, special=False), namespace="a")
    pair.upsert(ib[:m], B[:m], mb[:m], namespace="b")
    pair.each(lambda ix: ix.delete(delete_all=True, namespace="a"), "a")
    pair.upsert(ib[m:], B[m:], mb[m:], namespace="b")  # b's third page is one "a" gave back
    pl = pair.dev._ns["b"].pages
    assert pl == pair.plain._ns["b"].pages and len(pl) == 3 and pl != sorted(pl)
    nsf, ns_del = split_off_delete_filter(mf, index_filters(mf, mb, count=13, seed=51), mb)
    pair.compare(nsf, Q, namespace="b")
    out = {ib[i] for i in range(3, m, 5)}
    pair.each(lambda ix: ix.delete(ids=sorted(out), namespace="b"), "b")
    pair.compare(nsf, Q, namespace="b")
    removed = pair.delete_by_filter(ns_del, namespace="b")
    assert removed == sum(map(mf.compile_filter(ns_del), [x for i, x in zip(ib, mb) if i not in out])) > 0
    pair.compare(nsf, Q, namespace="b")
    st = pair.check_paths()  # every one of those misses was a device one
    assert st["demoted"] == {} and st["device"] == corpus.FIELDS and st["device_evals"] == len(pair.seen) == 98  # 5 x 12 + 1 in "", 3 x 12 + 1 in "b"
    assert pair.nonempty > len(pair.seen) // 2


def test_demotion_and_the_host_fallback(idxmod, mf, cuda):
    n = 300
    X, Q = vectors(n, 61), vectors(4, 62)
    metas = corpus.gen_metas(n, seed=63, special=False)
    for i, m in enumerate(metas):
        m["extra"] = i % 7                       # not indexed
        if i % 2:
            m["labels"] = ["x", "y"][: 1 + i % 3 % 2] + [i % 5]   # indexed, but a list
    ids = [f"v{i}" for i in range(n)]
    pair = Pair(idxmod, cuda, 1, fields=corpus.FIELDS + ["labels"], name="demote")
    pair.upsert(ids, X, metas)
    st = pair.dev.metadata_index_stats()
    assert list(st["demoted"]) == ["labels"] and "list" in st["demoted"]["labels"] and st["device"] == corpus.FIELDS
    host_filters = [{"labels": "x"}, {"labels": {"$in": ["y", 3]}}, {"labels": {"$nin": [4]}}, {"extra": {"$lt": 3}},
                    {"$or": [{"extra": 6}, {"color": "red"}]}, {"color": "red", "labels": {"$ne": "y"}}]
    pair.compare(host_filters, Q)
    st = pair.check_paths(host=len(host_filters))
    assert st["device_evals"] == 0
    dev_filters = index_filters(mf, metas, count=6, seed=64)
    pair.compare(dev_filters, Q)
    st = pair.check_paths(host=len(host_filters))
    assert st["device_evals"] == len(dev_filters)
    # a field demotes in mid-life: the same filter goes from the device to the host
    flt = {"size": {"$gte": 1}}
    pair.compare([flt], Q)
    pair.upsert(["late"], vectors(1, 65), [{"size": (1, 2), "color": "red"}])
    pair.compare([flt, {"color": "red"}], Q)
    st = pair.check_paths(host=len(host_filters) + 1)
    assert set(st["demoted"]) == {"labels", "size"} and "tuple" in st["demoted"]["size"]
    assert st["device"] == [f for f in corpus.FIELDS if f != "size"]
    assert pair.delete_by_filter({"labels": "x"}) > 0 and pair.delete_by_filter({"flag": True}) > 0
    pair.check_paths(host=len(host_filters) + 2)


def test_a_failed_column_write_sends_every_filter_to_the_host(idxmod, mf, mc, cuda, monkeypatch):
    n = 200
    X, Q = vectors(n, 71), vectors(4, 72)
    metas = corpus.gen_metas(n, seed=73, special=False)
    ids = [f"v{i}" for i in range(n)]
    pair = Pair(idxmod, cuda, 1, name="invalid")
    pair.upsert(ids, X, metas)
    filters = index_filters(mf, metas, count=4, seed=74)
    pair.compare(filters[:1], Q)
    assert pair.dev.metadata_index_stats()["device_evals"] == 1

    def boom(self, rows, tags, vals):
        raise RuntimeError("column write failed")

    import torch

    with monkeypatch.context() as mp:
        mp.setattr(mc.Columns, "write", boom)
        with pytest.raises(RuntimeError, match="column write failed"):
            pair.dev.upsert_tensor(["z0"], torch.from_numpy(vectors(1, 75)).cuda(), [{"color": "blue"}])
    assert "z0" not in pair.dev._rows and len(pair.dev) == n   # the host maps were not committed
    st = pair.dev.metadata_index_stats()
    assert st["valid"] is False and st["device_evals"] == 1
    # from now on the columns are never read, whatever is upserted; answers stay right
    pair.upsert(["z1"], vectors(1, 76), [{"color": "blue", "size": 3}])
    for flt in filters:
        got = [ix.query(vector=Q[0].tolist(), top_k=10, filter=flt) for ix in (pair.dev, pair.plain)]
        assert got[0] == got[1]
    st = pair.dev.metadata_index_stats()
    assert st["valid"] is False and st["device_evals"] == 1 and st["host_evals"] == len(filters)


def test_save_and_load_keep_the_config_and_the_answers(idxmod, mf, cuda, tmp_path):
    n = 400
    X, Q = vectors(n, 81), vectors(4, 82)
    metas = corpus.gen_metas(n, seed=83, special=False)
    ids = [f"v{i}" for i in range(n)]
    pair = Pair(idxmod, cuda, 2, name="snap")
    pair.upsert(ids, X, metas)
    pair.upsert([f"s{i}" for i in range(300)], vectors(300, 84), metas[:300], namespace="side")
    filters = index_filters(mf, metas, count=6, seed=85)
    d1, d2 = str(tmp_path / "with"), str(tmp_path / "without")
    pair.dev.save(d1)
    pair.plain.save(d2)
    man1, man2 = json.load(open(os.path.join(d1, "manifest.json"))), json.load(open(os.path.join(d2, "manifest.json")))
    assert man1["metadata_config"] == {"indexed": corpus.FIELDS}
    # without the config the manifest is what it always was: the same keys, in the same order
    assert list(man2) == ["format", "name", "dimension", "metric", "dtype", "ld", "count", "capacity", "filter", "ids",
                          "metadata", "namespaces"]
    del man1["metadata_config"]
    assert man1 == man2
    back = idxmod.Index.load(d1, devices=[cuda])           # the manifest's config, another shard count
    assert back.metadata_config == {"indexed": corpus.FIELDS}
    none = idxmod.Index.load(d2, devices=[cuda])
    assert none.metadata_config is None and none._cols is None
    late = idxmod.Index.load(d2, devices=[cuda], metadata_config={"indexed": ["color", "size"]})
    assert late.metadata_index_stats()["device"] == ["color", "size"]
    for ns in ("", "side"):
        for flt in filters:
            want = pair.plain.query(vector=Q[1].tolist(), top_k=10, filter=flt, namespace=ns)
            for ix in (back, none, late):
                got = ix.query(vector=Q[1].tolist(), top_k=10, filter=flt, namespace=ns)
                assert [m["id"] for m in got["matches"]] == [m["id"] for m in want["matches"]]
                assert np.allclose([m["score"] for m in got["matches"]], [m["score"] for m in want["matches"]], rtol=0, atol=1e-6)
    st = back.metadata_index_stats()
    assert st["valid"] and st["host_evals"] == 0 and st["device_evals"] == 2 * len(filters) and st["demoted"] == {}
    st = late.metadata_index_stats()  # only filters over color and size alone compile there; the rest fall back
    assert st["device_evals"] + st["host_evals"] == 2 * len(filters)
    assert none.metadata_index_stats() == {"indexed": [], "device": [], "demoted": {}, "valid": False, "device_evals": 0,
                                           "host_evals": 0}
    again = str(tmp_path / "again")
    back.save(again)
    assert json.load(open(os.path.join(again, "manifest.json")))["metadata_config"] == {"indexed": corpus.FIELDS}
