"""CPU tests of the float8 (OCP e4m3fn) index dtype's names and sizes: the C header, the ctypes
layer and the element-size helper agree, and an unknown dtype still raises."""
import os
import re

import pytest

from conftest import REPO, import_pkg


@pytest.fixture(scope="module")
def lib():
    return import_pkg("_lib")


def header_value(name):
    text = open(os.path.join(REPO, "include", "retrieval_core.h")).read()
    m = re.search(rf"^#define\s+{name}\s+(\d+)\s*$", text, flags=re.M)
    assert m, f"{name} is not defined in retrieval_core.h"
    return int(m.group(1))


def test_header_and_binding_agree(lib):
    assert header_value("RC_F8") == lib.RC_F8
    for name in ("RC_F32", "RC_F16", "RC_BF16"):  # the existing dtypes keep their values
        assert header_value(name) == getattr(lib, name)
    assert len({lib.RC_F32, lib.RC_F16, lib.RC_BF16, lib.RC_F8}) == 4
    assert header_value("RC_ABI_VERSION") == 1


def test_both_names_map_to_f8(lib):
    assert lib.DTYPES["float8_e4m3fn"] == lib.RC_F8
    assert lib.DTYPES["f8"] == lib.RC_F8
    assert lib.is_f8("f8") and lib.is_f8("float8_e4m3fn")
    assert not any(lib.is_f8(d) for d in ("float32", "f32", "float16", "f16", "bfloat16", "bf16", "int8"))


def test_element_size_helper(lib):
    want = {"float8_e4m3fn": 1, "f8": 1, "float16": 2, "f16": 2, "bfloat16": 2, "bf16": 2, "float32": 4, "f32": 4}
    assert set(want) == set(lib.DTYPES)
    for name, size in want.items():
        assert lib.dtype_bytes(name) == size, name


@pytest.mark.parametrize("name", ["float8", "float8_e5m2", "float8_e4m3fnuz", "int8", "", "F8"])
def test_unknown_dtype_raises(lib, name):
    assert name not in lib.DTYPES
    with pytest.raises(ValueError):
        lib.dtype_bytes(name)
