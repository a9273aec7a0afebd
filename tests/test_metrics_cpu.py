"""The metric entry points' argument checks return before any device call (CPU-only host), and
the binding names Pinecone's three metrics."""
import ctypes

import pytest

from conftest import import_pkg


@pytest.fixture(scope="module")
def L():
    return import_pkg("_lib")


def test_binding_names_the_three_metrics(L):
    assert set(L.METRICS) == {"cosine", "dotproduct", "euclidean"}
    assert {"rc_index_set_metric", "rc_index_get_metric", "rc_sharded_set_metric"} <= set(L.SIGNATURES)


def test_null_handles_are_invalid_without_touching_hip(L):
    lib = L.load()
    for metric in (L.METRICS["dotproduct"], 7):
        assert lib.rc_index_set_metric(None, metric) == L.RC_ERR_INVALID
        assert lib.rc_sharded_set_metric(None, metric) == L.RC_ERR_INVALID
    m = ctypes.c_int(-1)
    assert lib.rc_index_get_metric(None, ctypes.byref(m)) == L.RC_ERR_INVALID and m.value == -1
    with pytest.raises(ValueError):
        L.check(lib.rc_index_set_metric(None, L.METRICS["euclidean"]))
