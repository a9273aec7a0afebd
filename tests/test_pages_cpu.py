"""``pages.py`` (the named namespaces' page allocator and position <-> pool-row maps) and the
page-table entry points of the C ABI, on a host without a GPU."""
import ctypes
import os
import re

import pytest

from conftest import REPO, import_pkg

P = 256


@pytest.fixture(scope="module")
def pages():
    return import_pkg("pages")


@pytest.fixture(scope="module")
def lib():
    return import_pkg("_lib").load()


def test_page_rows_is_the_headers(pages):
    src = open(os.path.join(REPO, "include", "retrieval_core.h")).read()
    assert int(re.search(r"#define RC_PAGE_ROWS (\d+)", src).group(1)) == pages.PAGE_ROWS == import_pkg("_lib").RC_PAGE_ROWS == P


def test_pages_needs_no_torch():
    src = open(import_pkg("pages").__file__).read()
    assert "import torch" not in src and "import numpy" not in src


# ---------------------------------------------------------------- allocator --
def test_alloc_hands_out_fresh_pages_in_order_then_reuses_freed_ones(pages):
    a = pages.PageAllocator(8)
    assert a.alloc(3) == [0, 1, 2] and a.alloc(1) == [3]
    assert (a.high_water, a.used_pages, a.free_pages) == (4, 4, 4)
    a.free([1, 3])
    assert (a.used_pages, a.free_pages) == (2, 6)
    assert a.alloc(3) == [1, 3, 4]  # freed pages first, lowest first, then past the high-water mark
    assert a.high_water == 5
    assert a.alloc(0) == []


def test_free_refuses_what_is_not_allocated(pages):
    a = pages.PageAllocator(4)
    a.alloc(2)
    for bad in ([2], [-1], [0, 0]):
        with pytest.raises(ValueError):
            a.free(bad)
    a.free([0])
    with pytest.raises(ValueError):
        a.free([0])
    assert a.alloc(1) == [0]  # the refused calls freed nothing else
    assert a.used_pages == 2


def test_growth_request(pages):
    a = pages.PageAllocator(4)
    assert a.pages_short(4) == 0 and a.pages_short(5) == 1
    a.alloc(4)
    assert a.pages_short(1) == 1
    with pytest.raises(MemoryError):
        a.alloc(1)
    assert a.capacity_needed(0, 4 * P) == 4 * P         # nothing to do
    assert a.capacity_needed(1, 4 * P) == 8 * P         # doubling
    assert a.capacity_needed(13, 4 * P) == 32 * P       # ... until it fits (17 pages)
    assert a.capacity_needed(1, 1000) % P == 0          # a whole number of pages, whatever the pool had
    a.free([2])
    assert a.capacity_needed(1, 4 * P) == 4 * P         # a freed page serves it
    a.set_capacity(8)
    assert a.alloc(3) == [2, 4, 5]
    with pytest.raises(ValueError):
        a.set_capacity(7)


# --------------------------------------------------------------------- maps --
@pytest.mark.parametrize("S", [1, 3, 8])
def test_position_row_round_trip(pages, S):
    L = [5, 2, 9, 0, 7]
    sp = pages.span(S)
    assert sp == P * S
    n = 4 * sp + 77
    rows = pages.positions_to_rows(L, range(n), S)
    assert len(set(rows)) == n
    for i in list(range(0, n, 97)) + [sp - 1, sp, sp + 1, n - 1]:
        g = pages.position_to_row(L, i, S)
        assert g == rows[i] == L[i // sp] * sp + i % sp
        assert g % S == i % S                                   # the same shard in both spaces
        assert g // S == L[(i // S) // P] * P + (i // S) % P    # local row = page * 256 + local position % 256
        assert pages.row_to_position(L, g, S) == i
    with pytest.raises(ValueError):
        pages.position_to_row(L, 5 * sp, S)
    with pytest.raises(ValueError):
        pages.position_to_row(L, -1, S)
    with pytest.raises(ValueError):
        pages.row_to_position(L, 3 * sp, S)  # page 3 is not in the list


@pytest.mark.parametrize("S", [1, 3, 8])
def test_page_count_around_every_page_edge(pages, S):
    sp = P * S
    assert pages.pages_for(0, S) == 0
    for e in range(1, 5):
        assert pages.pages_for(e * sp - 1, S) == e
        assert pages.pages_for(e * sp, S) == e
        assert pages.pages_for(e * sp + 1, S) == e + 1
    assert pages.pages_for(1, S) == 1
    with pytest.raises(ValueError):
        pages.pages_for(-1, S)
    with pytest.raises(ValueError):
        pages.span(0)


def test_row_runs_coalesce_consecutive_pages(pages):
    S = 3
    sp = P * S
    assert pages.row_runs([4, 5, 6, 1, 2], 4 * sp + 10, S) == [(0, 4 * sp, 3 * sp), (3 * sp, 1 * sp, sp + 10)]
    assert pages.row_runs([5, 2], sp + 1, S) == [(0, 5 * sp, sp), (sp, 2 * sp, 1)]
    assert pages.row_runs([7], 5, S) == [(0, 7 * sp, 5)]
    assert pages.row_runs([], 0, S) == []
    # every position exactly once, at its own row
    L = [3, 4, 9, 10, 11, 0]
    n = 5 * sp + 100
    seen = {}
    for pos0, row0, cnt in pages.row_runs(L, n, S):
        for j in range(cnt):
            seen[pos0 + j] = row0 + j
    assert [seen[i] for i in range(n)] == pages.positions_to_rows(L, range(n), S)


# ---------------------------------------------------------------------- ABI --
NEW = ["rc_index_pages_set", "rc_index_search_pages", "rc_sharded_pages_set", "rc_sharded_search_pages",
       "rc_sharded_query_host_pages"]


def test_page_table_entry_points_are_declared_exported_and_bound(lib):
    src = open(os.path.join(REPO, "include", "retrieval_core.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = import_pkg("_lib")
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(raw, name), name
        assert name in L.SIGNATURES and getattr(lib, name).argtypes is not None
    assert lib.rc_abi_version() == 1
    assert getattr(lib, "rc_missing_symbols", ()) == ()


def test_page_table_calls_refuse_bad_arguments_before_any_device_call(lib):
    """RC_ERR_INVALID on a host without a GPU: the checks that need no handle state (a handle
    cannot be made here).  The pointers are never dereferenced.  The checks against a handle's
    own state — an unknown slot, n_pos beyond the table, a page past the capacity — run before
    any device call too, and are exercised where a handle exists (test_paged_scan_gpu.py)."""
    L = import_pkg("_lib")
    buf = (ctypes.c_int32 * 4)(0, 1, 2, 3)
    p = ctypes.cast(buf, ctypes.c_void_p)
    h = ctypes.c_void_p(0)
    INV = L.RC_ERR_INVALID
    assert lib.rc_index_pages_set(h, 0, p, 1, None) == INV and b"null index" in lib.rc_last_error()
    assert lib.rc_sharded_pages_set(h, 0, p, 1) == INV and b"null index" in lib.rc_last_error()
    assert lib.rc_index_search_pages(h, p, 1, 0, 1, 5, None, p, p, None) == INV
    assert lib.rc_sharded_search_pages(h, p, 1, 0, 1, 5, None, p, p, None) == INV
    assert lib.rc_sharded_query_host_pages(h, p, 1, 0, 1, 5, 0, None, p, p, None) == INV
    # a non-null (never dereferenced before these checks) handle: slot, counts, k and buffers
    fake = ctypes.cast((ctypes.c_char * 8192)(), ctypes.c_void_p)
    for slot in (-1, 1 << 20):
        assert lib.rc_index_pages_set(fake, slot, p, 1, None) == INV and b"slot" in lib.rc_last_error()
        assert lib.rc_sharded_pages_set(fake, slot, p, 1) == INV and b"slot" in lib.rc_last_error()
    assert lib.rc_index_pages_set(fake, 0, p, -1, None) == INV and b"negative" in lib.rc_last_error()
    assert lib.rc_sharded_pages_set(fake, 0, None, 2) == INV and b"null" in lib.rc_last_error()
    assert lib.rc_index_pages_set(fake, 0, None, 2, None) == INV and b"null" in lib.rc_last_error()
    for k in (0, 257):
        assert lib.rc_index_search_pages(fake, p, 1, 0, 1, k, None, p, p, None) == INV and b"top_k" in lib.rc_last_error()
        assert lib.rc_sharded_search_pages(fake, p, 1, 0, 1, k, None, p, p, None) == INV and b"top_k" in lib.rc_last_error()
        assert lib.rc_sharded_query_host_pages(fake, p, 1, 0, 1, k, 0, None, p, p, None) == INV and b"top_k" in lib.rc_last_error()
    assert lib.rc_index_search_pages(fake, p, -1, 0, 1, 5, None, p, p, None) == INV
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.rc_index_search_pages(fake, args[0], 1, 0, 1, 5, None, args[1], args[2], None) == INV
        assert b"null buffer" in lib.rc_last_error()
        assert lib.rc_sharded_search_pages(fake, args[0], 1, 0, 1, 5, None, args[1], args[2], None) == INV
        assert lib.rc_sharded_query_host_pages(fake, args[0], 1, 0, 1, 5, 0, None, args[1], args[2], None) == INV
    assert lib.rc_sharded_query_host_pages(fake, p, 1, 0, 1, 5, 1, None, p, p, None) == INV  # values wanted, none given
    assert lib.rc_sharded_query_host_pages(fake, p, 1, -1, 1, 5, 0, None, p, p, None) == INV
    assert lib.rc_sharded_query_host_pages(fake, p, 1, 0, -1, 5, 0, None, p, p, None) == INV
