"""The radix selection's interface without a GPU: ``deep_select`` is validated before anything is
made, the two entry points are bound and exported, and ``Config`` reads the variable."""
import ctypes
import importlib.util

import pytest

from conftest import import_pkg


@pytest.mark.parametrize("bad", ["auto", "", "Radix", 1, None, True])
def test_a_bad_deep_select_raises_naming_the_two_values(bad):
    idxmod = import_pkg("index")
    with pytest.raises(ValueError, match="'rounds' or 'radix'"):
        idxmod.Index("x", dimension=8, max_top_k=1000, deep_select=bad)


@pytest.mark.parametrize("name", ["rc_index_set_deep_select", "rc_sharded_set_deep_select"])
def test_the_entry_points_are_bound_exported_and_check_their_handle(name):
    L = import_pkg("_lib")
    lib = L.load()
    assert name in L.SIGNATURES and name not in lib.rc_missing_symbols
    assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
    assert (L.RC_DEEP_SELECT_ROUNDS, L.RC_DEEP_SELECT_RADIX) == (0, 1)
    assert getattr(lib, name)(None, L.RC_DEEP_SELECT_RADIX) == L.RC_ERR_INVALID


def test_config_reads_the_variable(monkeypatch):
    cfgmod = import_pkg("config")

    def fresh_config():  # a private copy of the module: the imported one stays as every other test sees it
        spec = importlib.util.spec_from_file_location("rc_config_probe", cfgmod.__file__)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod.Config

    monkeypatch.delenv("RC_INDEX_DEEP_SELECT", raising=False)
    assert fresh_config().INDEX_DEEP_SELECT == "rounds"
    monkeypatch.setenv("RC_INDEX_DEEP_SELECT", "radix")
    assert fresh_config().INDEX_DEEP_SELECT == "radix"
