"""The MXFP8 MLP's entry points on a host without a GPU: declared, exported, bound, and every
refusal made before any device call (the dummy pointers are never dereferenced)."""
import ctypes
import os
import re

import pytest

from conftest import REPO, import_pkg

NAMES = ["rc_model_set_mlp_dtype", "rc_model_get_mlp_dtype", "rc_mxfp8_quantize", "rc_gemm_mxfp8"]


@pytest.fixture(scope="module")
def lib():
    return import_pkg("_lib").load()


@pytest.mark.parametrize("name", NAMES)
def test_entry_is_declared_exported_and_bound(lib, name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "retrieval_core.h")).read(), flags=re.S)
    assert re.search(rf"\b{name}\s*\(", header)
    assert hasattr(ctypes.CDLL(import_pkg("_lib").LIB_PATH), name)
    assert name in import_pkg("_lib").SIGNATURES and getattr(lib, name).argtypes is not None


def test_set_mlp_dtype_refuses_null_model_and_unknown_kind(lib):
    L = import_pkg("_lib")
    fake = ctypes.cast((ctypes.c_uint8 * 64)(), ctypes.c_void_p)
    assert lib.rc_model_set_mlp_dtype(None, 1) == L.RC_ERR_INVALID
    assert lib.rc_model_set_mlp_dtype(fake, 7) == L.RC_ERR_INVALID
    assert b"mlp dtype" in lib.rc_last_error()


@pytest.mark.parametrize("null,N,K", [(0, 768, 3072), (2, 768, 3072), (4, 768, 3072), (None, 768, 96), (None, 100, 3072)])
def test_gemm_mxfp8_refuses_bad_arguments_before_any_device_call(lib, null, N, K):
    L = import_pkg("_lib")
    p = ctypes.cast((ctypes.c_uint8 * 64)(), ctypes.c_void_p)
    ops = [None if i == null else p for i in range(5)]  # A8, As, W8, Ws, bias
    assert lib.rc_gemm_mxfp8(*ops, 300, N, K, p, 197, None) == L.RC_ERR_INVALID
    assert lib.rc_gemm_mxfp8(p, p, p, p, p, 300, 768, 3072, None, 197, None) == L.RC_ERR_INVALID  # null out


def test_embedder_argument_check():
    vit = import_pkg("vit")
    assert vit.mlp_dtype_kind("bf16") == 0 and vit.mlp_dtype_kind("mxfp8") == 1
    with pytest.raises(ValueError):
        vit.mlp_dtype_kind("int4")
