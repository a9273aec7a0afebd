"""The swap-remove plan of ``Index.delete`` (``compaction.plan_compaction``) and the argument
checks of the two row-move entry points that return before any device call.  No GPU."""
import ctypes
import random
from collections import Counter

import pytest

from conftest import import_pkg


@pytest.fixture(scope="module")
def plan():
    return import_pkg("compaction").plan_compaction


def check_plan(plan, n, dead, n_shards):
    src, dst = plan(n, dead, n_shards)
    dead = set(dead)
    new_n = n - len(dead)
    holes = sorted(r for r in dead if r < new_n)
    survivors = sorted(r for r in range(new_n, n) if r not in dead)
    assert dst == holes                      # exactly the holes, ascending
    assert sorted(src) == survivors          # exactly the tail survivors
    assert len(src) == len(dst) and not set(src) & set(dst)
    hs = Counter(r % n_shards for r in holes)
    ss = Counter(r % n_shards for r in survivors)
    same = sum(1 for s, d in zip(src, dst) if s % n_shards == d % n_shards)
    assert same == sum(min(hs[s], ss[s]) for s in range(n_shards))
    # applied to the rows themselves, then truncated: every survivor exactly once
    rows = list(range(n))
    for s, d in zip(src, dst):
        rows[d] = rows[s]
    del rows[new_n:]
    assert sorted(rows) == sorted(set(range(n)) - dead)
    return src, dst


@pytest.mark.parametrize("n_shards", [1, 3, 8])
def test_random_plans(plan, n_shards):
    rng = random.Random(1000 + n_shards)
    for _ in range(200):
        n = rng.randint(0, 300)
        k = rng.choice([0, 1, n // 10, n // 2, n - 1, n]) if n else 0
        k = max(0, min(n, k))
        check_plan(plan, n, rng.sample(range(n), k), n_shards)


@pytest.mark.parametrize("n_shards", [1, 3, 8])
def test_edge_cases(plan, n_shards):
    assert check_plan(plan, 100, [], n_shards) == ([], [])
    assert check_plan(plan, 100, range(90, 100), n_shards) == ([], [])  # the whole tail: no moves
    assert check_plan(plan, 100, range(100), n_shards) == ([], [])      # everything
    assert check_plan(plan, 100, [50], n_shards) == ([99], [50])         # one row in the middle
    assert check_plan(plan, 100, [99], n_shards) == ([], [])
    assert check_plan(plan, 0, [], n_shards) == ([], [])
    assert plan(100, [50, 50, 50], n_shards) == ([99], [50])             # repeats count once


def test_same_shard_pairs_come_first(plan):
    # 3 shards, n = 12: holes 0 and 1 (shards 0, 1); the tail [10, 12) survives whole: 10 (shard 1), 11 (shard 2)
    src, dst = plan(12, [0, 1], 3)
    assert dst == [0, 1] and src == [11, 10]  # hole 1 takes its own shard's row 10, hole 0 what is left


def test_bad_rows_rejected(plan):
    for bad in ([-1], [10], [3, 11]):
        with pytest.raises(ValueError):
            plan(10, bad, 3)
    with pytest.raises(ValueError):
        plan(10, [1], 0)


def test_cost_does_not_scale_with_n(plan):
    """10 rows out of 100M: the plan only looks at the deleted rows and the 10-row tail (a walk of
    100M entries would take seconds and gigabytes; this is instant)."""
    n = 100_000_000
    dead = [5, 77, 1_000_003, 50_000_000, 99_999_990, 99_999_995, 99_999_999, 12, 13, 14]
    src, dst = plan(n, dead, 8)
    assert dst == [5, 12, 13, 14, 77, 1_000_003, 50_000_000]
    assert sorted(src) == [99_999_991, 99_999_992, 99_999_993, 99_999_994, 99_999_996, 99_999_997, 99_999_998]


def test_delete_images_rejects_bad_bodies_without_an_index():
    """/delete_images validates its JSON body before it opens the index: 422 without a list of
    string ids, and an empty list deletes nothing (no GPU needed for either)."""
    from fastapi.testclient import TestClient

    for app in (import_pkg("ingesting.main").app, import_pkg("service").app):
        c = TestClient(app)
        for bad in ({"json": {}}, {"json": {"ids": "abc"}}, {"json": {"ids": [1]}}, {"json": ["a"]}, {"content": b"{"}, {}):
            assert c.post("/delete_images", **bad).status_code == 422, bad
        r = c.post("/delete_images", json={"ids": []})
        assert r.status_code == 200 and r.json() == {"deleted_count": 0}


def test_move_rows_arguments_rejected_before_any_device_call():
    L = import_pkg("_lib")
    lib = L.load()
    buf = (ctypes.c_int64 * 4)(0, 1, 2, 3)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.rc_index_move_rows(None, p, p, 4, None) == L.RC_ERR_INVALID
    assert b"null index" in lib.rc_last_error()
    assert lib.rc_sharded_move_rows(None, p, p, 4) == L.RC_ERR_INVALID
    assert b"null index" in lib.rc_last_error()
    # n < 0 is refused before the handle is touched (any non-null value stands in for one)
    fake = ctypes.c_void_p(ctypes.addressof(buf))
    assert lib.rc_index_move_rows(fake, p, p, -1, None) == L.RC_ERR_INVALID
    assert b"negative" in lib.rc_last_error()
    assert lib.rc_sharded_move_rows(fake, p, p, -1) == L.RC_ERR_INVALID
    assert b"negative" in lib.rc_last_error()
