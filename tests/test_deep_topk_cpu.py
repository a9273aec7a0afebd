"""Deep top-k without a GPU: the new entry points are exported and bound, their argument errors
come back as RC_ERR_INVALID before any device call, ``Index(max_top_k=...)`` is validated before
anything is allocated, and ``Config.INDEX_MAX_TOP_K`` reaches ``get_index``."""
import ctypes
import importlib
import importlib.util
import os
import re

import pytest

from conftest import REPO, import_pkg

DEEP = ["rc_index_search_deep", "rc_index_search_pages_deep", "rc_sharded_search_deep", "rc_sharded_search_pages_deep",
        "rc_index_scores", "rc_index_scores_pages"]


@pytest.fixture(scope="module")
def L():
    return import_pkg("_lib")


@pytest.fixture(scope="module")
def lib(L):
    return L.load()


def header():
    return open(os.path.join(REPO, "include", "retrieval_core.h")).read()


def test_the_deep_calls_are_declared_exported_and_bound(L, lib):
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in DEEP:
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert hasattr(raw, name), name
        assert name in L.SIGNATURES and name not in lib.rc_missing_symbols
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    # the paged / sharded twins take their twins' arguments with the mode dropped
    assert len(L.SIGNATURES["rc_index_search_deep"][1]) == len(L.SIGNATURES["rc_index_search_masked"][1]) - 1
    assert len(L.SIGNATURES["rc_index_search_pages_deep"][1]) == len(L.SIGNATURES["rc_index_search_pages_ex"][1]) - 1
    assert len(L.SIGNATURES["rc_sharded_search_deep"][1]) == len(L.SIGNATURES["rc_sharded_search_masked"][1]) - 1
    assert len(L.SIGNATURES["rc_sharded_search_pages_deep"][1]) == len(L.SIGNATURES["rc_sharded_search_pages_ex"][1]) - 1


def test_the_limits_in_the_header_and_the_binding_agree(L):
    defs = dict(re.findall(r"#define (RC_[A-Z_]+) (\d+)", header()))
    assert int(defs["RC_TOPK_MAX"]) == L.RC_TOPK_MAX == 256  # unchanged
    assert int(defs["RC_DEEP_TOPK_MAX"]) == L.RC_DEEP_TOPK_MAX == 10000
    assert int(defs["RC_DEEP_SELECT_ROWS"]) == L.RC_DEEP_SELECT_ROWS


def test_argument_errors_come_back_without_a_device(L, lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    bad = L.RC_ERR_INVALID
    # a null handle, before anything else
    assert lib.rc_index_search_deep(None, p, 1, 10, 300, None, p, p, None) == bad
    assert b"null index" in lib.rc_last_error()
    assert lib.rc_index_search_pages_deep(None, p, 1, 0, 10, 300, None, p, p, None) == bad
    assert lib.rc_sharded_search_deep(None, p, 1, 10, 300, None, p, p, None) == bad
    assert lib.rc_sharded_search_pages_deep(None, p, 1, 0, 10, 300, None, p, p, None) == bad
    assert lib.rc_index_scores(None, p, 10, p, None) == bad
    assert lib.rc_index_scores_pages(None, p, 0, 10, p, None) == bad
    # the existing calls keep their own bound's message; the handle check comes first there too
    assert lib.rc_index_search_masked(None, p, 1, 10, 257, None, p, p, 1, None) == bad


def test_max_top_k_is_validated_before_anything_is_made(L):
    idxmod = import_pkg("index")
    for bad in (0, 255, 10001, -1, 256.0, "1000", None, True):
        with pytest.raises(ValueError, match="max_top_k"):
            idxmod.Index("x", dimension=8, max_top_k=bad)
    import inspect

    assert inspect.signature(idxmod.Index.__init__).parameters["max_top_k"].default == 256
    assert inspect.signature(idxmod.Index.load).parameters["max_top_k"].default == 256
    for cls in (idxmod.DeviceIndex, idxmod.ShardSet):
        assert callable(cls.search_deep) and callable(cls.search_pages_deep)
    assert callable(idxmod.DeviceIndex.scores)


def test_config_reads_the_environment_and_get_index_passes_it(monkeypatch):
    cfgmod = import_pkg("config")
    assert cfgmod.Config.INDEX_MAX_TOP_K == int(os.getenv("RC_INDEX_MAX_TOP_K", "256"))

    def fresh_config():  # a second, private copy of the module: the imported one stays as every other test sees it
        spec = importlib.util.spec_from_file_location("rc_config_probe", cfgmod.__file__)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod.Config

    monkeypatch.delenv("RC_INDEX_MAX_TOP_K", raising=False)
    assert fresh_config().INDEX_MAX_TOP_K == 256
    monkeypatch.setenv("RC_INDEX_MAX_TOP_K", "4000")
    assert fresh_config().INDEX_MAX_TOP_K == 4000
    # get_index hands Config.INDEX_MAX_TOP_K to the Index it makes
    utils = import_pkg("ingesting.utils")
    idxmod = import_pkg("index")
    seen = {}

    class Probe:
        def __init__(self, name, **kw):
            seen.update(kw)

    monkeypatch.setattr(idxmod, "Index", Probe)
    monkeypatch.setattr(utils.Config, "INDEX_MAX_TOP_K", 777)
    monkeypatch.setattr(utils, "_indexes", {})
    utils.get_index("deep-probe", devices=[None])
    assert seen["max_top_k"] == 777
