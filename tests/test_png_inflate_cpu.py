"""The device inflate's host side without a GPU: rc_png_decode / rc_png_decode_stats are declared,
exported and bound and refuse bad arguments before any device call, and png.parse's
inflate="device" form returns the joined IDAT bytes with the same chunk-level ValueErrors."""
import ctypes
import os
import struct
import zlib

import pytest

from conftest import REPO, import_pkg


def chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def make(parts, w=2, h=1):
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + b"".join(chunk(k, b) for k, b in parts) + chunk(b"IEND", b""))


Z = zlib.compress(b"\x00abcdef")


@pytest.fixture(scope="module")
def L():
    return import_pkg("_lib")


def test_entry_points_are_declared_exported_and_bound(L):
    header = open(os.path.join(REPO, "include", "retrieval_core.h")).read()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in ("rc_png_decode", "rc_png_decode_stats", "rc_png_decode_timing"):
        assert name + "(" in header and hasattr(raw, name) and name in L.SIGNATURES
    assert L.load().rc_missing_symbols == ()


def stream(L, z=Z, w=2, h=1, depth=8, color=2, size=None):
    s = L.PngStream()
    s.width, s.height, s.depth, s.color = w, h, depth, color
    s.idat, s.idat_bytes, s.out_offset = z, len(z) if size is None else size, 0
    return s


@pytest.mark.parametrize("what,status", [
    ("null_streams", "RC_ERR_INVALID"), ("null_rgb", "RC_ERR_INVALID"), ("null_flags", "RC_ERR_INVALID"),
    ("negative_n", "RC_ERR_INVALID"), ("zero_width", "RC_ERR_INVALID"), ("depth_3", "RC_ERR_INVALID"),
    ("depth_16", "RC_ERR_UNSUPPORTED"), ("short_stream", "RC_ERR_INVALID"), ("zlib_header", "RC_ERR_INVALID"),
    ("above_the_cap", "RC_ERR_UNSUPPORTED"), ("output_range", "RC_ERR_INVALID"),
])
def test_bad_arguments_are_refused_before_any_device_call(L, what, status):
    """No GPU here: a call that reached HIP would return RC_ERR_HIP.  The pointers are never read
    (rgb is a host buffer; the stream above the cap is 8 bytes long)."""
    lib = L.load()
    one = {"zero_width": dict(w=0), "depth_3": dict(depth=3), "depth_16": dict(depth=16), "short_stream": dict(size=5),
           "zlib_header": dict(z=b"\x79" + Z[1:]), "above_the_cap": dict(size=L.RC_PNG_INFLATE_MAX_BYTES + 1)}.get(what, {})
    streams = (L.PngStream * 1)(stream(L, **one))
    rgb, flags = (ctypes.c_uint8 * 256)(), (ctypes.c_int32 * 1)()
    args = [0, -1 if what == "negative_n" else 1, None if what == "null_streams" else streams,
            None if what == "null_rgb" else ctypes.addressof(rgb), 5 if what == "output_range" else 256,
            None if what == "null_flags" else flags, None]
    assert lib.rc_png_decode(*args) == getattr(L, status)
    a = ctypes.c_int64()
    assert lib.rc_png_decode_stats(0, None, ctypes.byref(a)) == L.RC_ERR_INVALID
    assert lib.rc_png_decode_timing(0, 0, None, ctypes.byref(a)) == L.RC_OK and a.value == 0  # off: no device call


def test_parse_returns_the_joined_idat_and_keeps_the_chunk_errors():
    png = import_pkg("png")
    good = make([(b"IDAT", Z[:3]), (b"IDAT", Z[3:4]), (b"IDAT", Z[4:])])
    got = png.parse(good, inflate="device")
    assert isinstance(got, png.PngStream) and got.idat == Z and got.palette is None and got.info[:2] == (2, 1)
    assert png.parse(good)[1] == b"\x00abcdef" == png.inflate_idat(got.info, got.idat)
    bad_crc = good[:-20] + bytes([good[-20] ^ 1]) + good[-19:]
    apart = make([(b"IDAT", Z[:3]), (b"tEXt", b"a\x00b"), (b"IDAT", Z[3:])])
    for data in (bad_crc, apart, make([])):  # CRC, chunk order, no IDAT: the same error, word for word
        with pytest.raises(ValueError) as host:
            png.parse(data)
        with pytest.raises(ValueError) as dev:
            png.parse(data, inflate="device")
        assert str(host.value) == str(dev.value)
    for data in (make([(b"IDAT", b"\x79" + Z[1:])]), make([(b"IDAT", Z[:5])])):  # zlib header, too short
        with pytest.raises(ValueError):
            png.parse(data, inflate="device")
