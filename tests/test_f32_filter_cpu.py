"""The float32 filter (RC_FILTER_F32) without a GPU: the binding and the header know the new kind, and
the constructor pairs it with float32 storage, under every metric, before any device work."""
import os
import re

import pytest

from conftest import REPO, import_pkg

METRICS = ["cosine", "dotproduct", "euclidean"]


class Reached(Exception):
    pass


def stop(*a, **k):  # in ShardSet's place: the constructor's validation let the arguments through
    raise Reached()


def test_binding_and_header_know_the_f32_filter():
    L = import_pkg("_lib")
    assert L.FILTERS["f32"] == 4 == L.RC_FILTER_F32
    assert (L.FILTERS["native"], L.FILTERS["i8"], L.FILTERS["f8"], L.FILTERS["metric"]) == (0, 1, 2, 3)  # unchanged
    src = open(os.path.join(REPO, "include", "retrieval_core.h")).read()
    assert re.search(r"^#define\s+RC_FILTER_F32\s+4\s*$", src, flags=re.M)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float8_e4m3fn", "f8"])
def test_the_f32_filter_needs_float32_storage(dtype, metric, monkeypatch):
    idx = import_pkg("index")
    monkeypatch.setattr(idx, "ShardSet", stop)
    with pytest.raises(ValueError, match="needs dtype='float32'"):
        idx.Index("x", dimension=64, dtype=dtype, metric=metric, filter="f32")


def test_the_paged_batched_search_keeps_refusing_float32(monkeypatch):
    idx = import_pkg("index")
    monkeypatch.setattr(idx, "ShardSet", stop)
    with pytest.raises(ValueError, match="paged_search"):
        idx.Index("x", dimension=64, dtype="float32", filter="f32", paged_search="mfma")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["float32", "f32"])
def test_every_metric_passes_validation_on_float32(dtype, metric, monkeypatch):
    idx = import_pkg("index")
    monkeypatch.setattr(idx, "ShardSet", stop)
    with pytest.raises(Reached):
        idx.Index("ok", dimension=64, dtype=dtype, metric=metric, filter="f32")
