"""The entropy-stage switch of the JPEG decoder: declared, exported, bound, and refusing bad
arguments before any device call."""
import ctypes

import pytest

from conftest import import_pkg
from test_abi_cpu import declared_functions

NAMES = {"rc_jpeg_decoder_set_entropy": 2, "rc_jpeg_decoder_get_entropy": 2, "rc_jpeg_decoder_entropy_stats": 3,
         "rc_jpeg_decoder_coefficients": 6, "rc_jpeg_decoder_upload_bytes": 2}


@pytest.mark.parametrize("name", list(NAMES))
def test_entry_is_declared_exported_and_bound(name):
    L = import_pkg("_lib")
    assert name in declared_functions()
    assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
    assert len(L.SIGNATURES[name][1]) == NAMES[name]
    assert len(getattr(L.load(), name).argtypes) == NAMES[name]


def test_null_handle_is_invalid():
    L = import_pkg("_lib")
    lib = L.load()
    kind, a, b = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.rc_jpeg_decoder_set_entropy(None, L.RC_JPEG_ENTROPY_DEVICE) == L.RC_ERR_INVALID
    assert lib.rc_jpeg_decoder_get_entropy(None, ctypes.byref(kind)) == L.RC_ERR_INVALID
    assert lib.rc_jpeg_decoder_entropy_stats(None, ctypes.byref(a), ctypes.byref(b)) == L.RC_ERR_INVALID
    assert lib.rc_jpeg_decoder_upload_bytes(None, ctypes.byref(a)) == L.RC_ERR_INVALID
    assert lib.rc_jpeg_decoder_coefficients(None, 0, None, None, None, None) == L.RC_ERR_INVALID


def test_unknown_entropy_is_a_value_error_before_the_library_loads(monkeypatch):
    jpeg = import_pkg("jpeg")
    monkeypatch.setattr(jpeg, "load", lambda: pytest.fail("the library was loaded"))
    with pytest.raises(ValueError, match="entropy"):
        jpeg.JpegDecoder(entropy="nope")


def test_gpu_huffman_is_off_by_default():
    assert import_pkg("config").Config.GPU_HUFFMAN is False
