"""The search mode of the mask inside the filter GEMM (``RC_SEARCH_MFMA_MASKED``): the constant in
the header and in ``_lib``, and the call's argument check.  No GPU."""
import os
import re

from conftest import import_pkg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_defines_the_mode_as_3():
    text = open(os.path.join(REPO, "include", "retrieval_core.h")).read()
    modes = dict(re.findall(r"^#define\s+(RC_SEARCH_\w+)\s+(\d+)", text, flags=re.M))
    assert modes == {"RC_SEARCH_AUTO": "0", "RC_SEARCH_SCAN": "1", "RC_SEARCH_MFMA": "2", "RC_SEARCH_MFMA_MASKED": "3"}


def test_lib_names_the_mode():
    L = import_pkg("_lib")
    assert L.RC_SEARCH_MFMA_MASKED == 3
    assert L.SEARCH_MODES["mfma_masked"] == 3
    assert L.SEARCH_MODES == {"auto": 0, "scan": 1, "mfma": 2, "mfma_masked": 3}


def test_a_null_handle_is_refused_under_the_new_mode():
    L = import_pkg("_lib")
    lib = L.load()
    st = lib.rc_index_search_masked(None, None, 1, 10, 5, None, None, None, L.RC_SEARCH_MFMA_MASKED, None)
    assert st == L.RC_ERR_INVALID
    assert b"null index" in lib.rc_last_error()  # the handle's error, not "unknown search mode"
