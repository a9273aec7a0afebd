"""The batched MFMA search over pages without a GPU: the two entry points and their argument
checks, the pinned set of search modes, and ``Index(..., paged_search=...)``'s validation, which
runs before any device work."""
import os
import re

import pytest

from conftest import import_pkg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_two_entry_points_are_exported_and_refuse_a_null_handle():
    L = import_pkg("_lib")
    lib = L.load()
    assert "rc_index_search_pages_ex" not in lib.rc_missing_symbols
    assert "rc_sharded_search_pages_ex" not in lib.rc_missing_symbols
    for fn in (lib.rc_index_search_pages_ex, lib.rc_sharded_search_pages_ex):
        for mode in (L.RC_SEARCH_AUTO, L.RC_SEARCH_SCAN, L.RC_SEARCH_MFMA, L.RC_SEARCH_MFMA_MASKED):
            assert fn(None, None, 1, 0, 10, 5, None, None, None, mode, None) == L.RC_ERR_INVALID
            assert b"null index" in lib.rc_last_error()
    assert lib.rc_abi_version() == 1


def test_an_unknown_mode_is_invalid():
    L = import_pkg("_lib")
    lib = L.load()
    for fn in (lib.rc_index_search_pages_ex, lib.rc_sharded_search_pages_ex):
        for mode in (-1, 4, 99):
            assert fn(None, None, 1, 0, 10, 5, None, None, None, mode, None) == L.RC_ERR_INVALID
            assert b"unknown search mode" in lib.rc_last_error()


def test_the_header_still_defines_exactly_the_four_modes():
    text = open(os.path.join(REPO, "include", "retrieval_core.h")).read()
    modes = dict(re.findall(r"^#define\s+(RC_SEARCH_\w+)\s+(\d+)", text, flags=re.M))
    assert modes == {"RC_SEARCH_AUTO": "0", "RC_SEARCH_SCAN": "1", "RC_SEARCH_MFMA": "2", "RC_SEARCH_MFMA_MASKED": "3"}
    for name in ("rc_index_search_pages_ex", "rc_sharded_search_pages_ex", "rc_index_search_pages", "rc_sharded_search_pages"):
        assert re.search(r"^int " + name + r"\(", text, flags=re.M), name
    assert import_pkg("_lib").SEARCH_MODES == {"auto": 0, "scan": 1, "mfma": 2, "mfma_masked": 3}


@pytest.mark.parametrize("kw", [{"paged_search": "fast"}, {"paged_search": None}, {"paged_search": "MFMA"},
                                {"paged_search": "mfma", "dtype": "float32"},
                                {"paged_search": "mfma", "dtype": "f8", "filter": "f8"},
                                {"paged_search": "mfma", "dtype": "float8_e4m3fn"},
                                {"paged_search": "mfma", "dtype": "float16", "filter": "i8"},
                                {"paged_search": "mfma", "dtype": "bfloat16", "filter": "f8"}])
def test_the_keyword_is_validated_before_any_device_work(kw, monkeypatch):
    idx = import_pkg("index")

    def no_device(*a, **k):
        raise AssertionError("the constructor reached the device")

    monkeypatch.setattr(idx, "ShardSet", no_device)
    with pytest.raises(ValueError, match="paged_search"):
        idx.Index("bad", dimension=64, **kw)


def test_the_accepted_values_reach_the_shard_set(monkeypatch):
    """"scan" and "mfma" (on f16 / bf16 with the native or the metric filter) pass the validation:
    the constructor goes on to make its ShardSet."""
    idx = import_pkg("index")

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()

    monkeypatch.setattr(idx, "ShardSet", stop)
    for kw in ({}, {"paged_search": "scan", "dtype": "float32"}, {"paged_search": "mfma", "dtype": "float16"},
               {"paged_search": "mfma", "dtype": "bfloat16", "filter": "metric", "metric": "euclidean"}):
        with pytest.raises(Reached):
            idx.Index("ok", dimension=64, **kw)
