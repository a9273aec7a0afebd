"""The streaming int8 filter (RC_FILTER_I8_STREAM) without a GPU: the header and the binding know the kind,
and the constructor refuses what it refuses of "i8", before any device work."""
import os
import re

import pytest

from conftest import REPO, import_pkg


def test_header_and_binding_know_the_kind():
    L = import_pkg("_lib")
    assert L.FILTERS["i8_stream"] == 5
    assert re.search(r"^#define\s+RC_FILTER_I8_STREAM\s+5\s*$", open(os.path.join(REPO, "include", "retrieval_core.h")).read(), flags=re.M)


def test_set_filter_checks_the_handle_not_the_kind():
    L = import_pkg("_lib")
    lib = L.load()
    assert lib.rc_index_set_filter(None, 5, None) == L.RC_ERR_INVALID
    assert b"null index" in lib.rc_last_error()


@pytest.mark.parametrize("kwargs", [{"paged_search": "mfma"}, {"metric": "dotproduct"}, {"dtype": "f8"}])
def test_constructor_refuses_what_it_refuses_of_i8(kwargs, monkeypatch):
    idx = import_pkg("index")
    monkeypatch.setattr(idx, "ShardSet", lambda *a, **k: pytest.fail("device work before validation"))
    for kind in ("i8", "i8_stream"):
        with pytest.raises(ValueError) as e:  # the kind is known: refused for what it is, as "i8" is
            idx.Index("x", dimension=64, filter=kind, **kwargs)
        assert "unknown filter" not in str(e.value)
