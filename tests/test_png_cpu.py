"""The PNG host stage (png.py: parser, inflate, validation) and the ABI of rc_png_reconstruct.
No GPU: everything here returns or raises before any device call."""
import ctypes
import struct
import zlib
from io import BytesIO

import numpy as np
import pytest
from PIL import Image

from conftest import import_pkg
from test_abi_cpu import declared_functions

P = import_pkg("png")


def chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def png(w, h, depth, color, raw, lace=0, extra=b"") -> bytes:
    return (P.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color, 0, 0, lace)) + extra
            + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


GOOD_RAW = b"\x00abcdef\x01ghijkl"  # 2 x 2 RGB: two rows of a filter byte and six data bytes


def test_probe_reads_the_header():
    assert P.probe(png(2, 2, 8, 2, GOOD_RAW)) == P.PngInfo(2, 2, 8, 2, 0, 1)
    b = BytesIO()
    Image.fromarray(np.zeros((5, 9), np.uint8)).convert("P").save(b, format="PNG")
    assert P.probe(b.getvalue())[:4] == (9, 5, 8, 3) and P.is_gpu_decodable(b.getvalue())
    info, raw, palette = P.parse(png(2, 2, 8, 2, GOOD_RAW))
    assert raw == GOOD_RAW and palette is None
    with pytest.raises(ValueError):
        P.probe(b"\xff\xd8\xff\xe0 not a png")
    assert not P.is_gpu_decodable(b"\xff\xd8\xff\xe0")


@pytest.mark.parametrize("data", [
    png(2, 2, 8, 2, b"\x00abc\x00def\x00ghijkl", lace=1),                        # Adam7: passes 1, 6 and 7
    png(1, 1, 16, 2, b"\x00" + bytes(6)),                                       # 16-bit samples
    png(2, 2, 8, 2, GOOD_RAW, extra=chunk(b"acTL", struct.pack(">II", 2, 0))),  # APNG
    png(P.MAX_UNITS + 1, 1, 8, 0, bytes(P.MAX_UNITS + 2)),                      # wider than the carry row
    png(8192, 2049, 1, 0, bytes(2049 * 1025)),                                  # above MAX_PIXELS (2^24)
], ids=["adam7", "16bit", "apng", "wide", "large"])
def test_out_of_scope_streams_stay_on_the_host(data):
    Image.open(BytesIO(data)).convert("RGB")  # valid for Pillow
    assert P.probe(data).supported == 0 and not P.is_gpu_decodable(data)
    with pytest.raises(P.PngUnsupported):
        P.parse(data)


def test_damaged_streams_raise_before_any_library_call(monkeypatch):
    monkeypatch.setattr(import_pkg("_lib"), "load", lambda: pytest.fail("the library was reached"))
    good = png(2, 2, 8, 2, GOOD_RAW)
    at = good.index(b"IDAT")
    size = struct.unpack(">I", good[at - 4:at])[0]
    cut = good[:at - 4] + chunk(b"IDAT", good[at + 4:at + 4 + size - 5]) + chunk(b"IEND", b"")
    flipped = good[:at + 6] + bytes([good[at + 6] ^ 1]) + good[at + 7:]
    for bad in (cut, flipped, png(2, 2, 8, 2, GOOD_RAW + b"m"), png(2, 2, 8, 2, GOOD_RAW[:-1]),
                png(2, 2, 8, 2, GOOD_RAW.replace(b"\x01", b"\x07")), good[:-12], png(2, 2, 8, 3, b"\x00ab\x00cd")):
        with pytest.raises(ValueError) as e:
            P.parse(bad)
        assert not isinstance(e.value, P.PngUnsupported)
    one, other = P.stage([good, cut], tolerant=True)  # the services' form: a bad image fails on its own
    assert one[1] == GOOD_RAW and isinstance(other, ValueError)


def test_entry_point_is_exported_declared_and_checks_its_arguments():
    L = import_pkg("_lib")
    lib = L.load()
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "rc_png_reconstruct")
    assert "rc_png_reconstruct" in declared_functions() and "rc_png_reconstruct" in L.SIGNATURES
    im = (L.PngImage * 1)()
    im[0].width, im[0].height, im[0].depth, im[0].color = 2, 2, 8, 2
    im[0].scanlines, im[0].scan_bytes = GOOD_RAW, len(GOOD_RAW)
    for field, value, what in (("scan_bytes", 13, b"stride"), ("scanlines", GOOD_RAW.replace(b"\x01", b"\x07"), b"filter"),
                               ("out_offset", 1, b"output")):
        keep = getattr(im[0], field)
        setattr(im[0], field, value)
        assert lib.rc_png_reconstruct(0, 1, im, 4096, 12, None) == L.RC_ERR_INVALID and what in lib.rc_last_error()
        setattr(im[0], field, keep)
    for field, value in (("depth", 16), ("height", 1 << 24)):  # 16-bit; 2 x 2^24 pixels
        keep = getattr(im[0], field)
        setattr(im[0], field, value)
        assert lib.rc_png_reconstruct(0, 1, im, 4096, 12, None) == L.RC_ERR_UNSUPPORTED
        setattr(im[0], field, keep)
