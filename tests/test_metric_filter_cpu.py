"""The metric filter (RC_FILTER_METRIC) without a GPU: the binding and the header know the new
kind, the library refuses it on a null handle before any device call, and the constructor pairs it
with the dtypes its filter GEMM can read.
"""
import os
import re

import pytest

from conftest import REPO, import_pkg

HEADER = os.path.join(REPO, "include", "retrieval_core.h")


def test_binding_and_header_know_the_metric_filter():
    L = import_pkg("_lib")
    assert L.FILTERS["metric"] == 3 == L.RC_FILTER_METRIC
    assert (L.FILTERS["native"], L.FILTERS["i8"], L.FILTERS["f8"]) == (0, 1, 2)  # the earlier kinds keep their values
    src = open(HEADER).read()
    assert re.search(r"^#define\s+RC_FILTER_METRIC\s+3\s*$", src, flags=re.M)
    assert re.search(r"^#define\s+RC_ABI_VERSION\s+1\s*$", src, flags=re.M)  # an addition: the ABI version stays


def test_set_filter_on_a_null_index_is_invalid():
    """Argument validation comes first: no HIP call is made (this machine may have no GPU)."""
    L = import_pkg("_lib")
    lib = L.load()
    assert lib.rc_index_set_filter(None, L.RC_FILTER_METRIC, None) == L.RC_ERR_INVALID
    assert lib.rc_index_set_filter(None, 4, None) == L.RC_ERR_INVALID


def test_index_constructor_pairs_the_metric_filter_with_f16_and_bf16():
    """Refused before any device call: "metric" on f32 and float8 storage, under every metric; and
    the cosine-only kinds stay refused on a non-cosine index."""
    idxmod = import_pkg("index")
    for dtype in ("float32", "f32", "float8_e4m3fn", "f8"):
        for metric in ("cosine", "dotproduct", "euclidean"):
            # the dtype check's own message: "metric" is a known kind, refused for this storage
            with pytest.raises(ValueError, match="needs dtype float16 or bfloat16"):
                idxmod.Index("x", dimension=64, dtype=dtype, metric=metric, filter="metric")
    for flt in ("i8", "f8"):
        with pytest.raises(ValueError, match="cosine-only"):
            idxmod.Index("x", dimension=64, dtype="float16", metric="dotproduct", filter=flt)
