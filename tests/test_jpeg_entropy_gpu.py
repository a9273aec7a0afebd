"""The device entropy stage (JpegDecoder(entropy="device")) against the host Huffman decoder of
the same library: integer work, so coefficients and pixels are compared for equality."""
import numpy as np
import pytest
import torch

import jpeg_cases
from conftest import import_pkg

pytestmark = pytest.mark.gpu

CASES = dict(jpeg_cases.cases())


@pytest.fixture(scope="module")
def jpeg(cuda):
    return import_pkg("jpeg")


@pytest.fixture(scope="module")
def dev(jpeg):
    return jpeg.JpegDecoder(device=0, max_images=128, entropy="device")


@pytest.fixture(scope="module")
def host(jpeg):
    return jpeg.JpegDecoder(device=0, max_images=128, entropy="host")


def scan_bytes(data: bytes) -> int:
    """Bytes between the SOS header and EOI (stuffing and restart markers included)."""
    sos = data.index(b"\xff\xda")
    return len(data) - 2 - (sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big"))


def check_device_decoded(jpeg, dev, data):
    before = dev.entropy_stats()
    (got,) = dev.coefficients([data])
    after = dev.entropy_stats()
    assert np.array_equal(got, jpeg.decode_coefficients(data)[1])
    assert after["device_images"] == before["device_images"] + 1
    assert after["host_fallbacks"] == before["host_fallbacks"]


@pytest.mark.parametrize("name", list(CASES))
def test_coefficients_bit_for_bit(jpeg, dev, name):
    check_device_decoded(jpeg, dev, CASES[name])


@pytest.mark.parametrize("rows", [0, 1], ids=["one_segment", "restart_rows"])
def test_scan_spanning_several_workgroups(jpeg, dev, rows):
    """The passes between workgroups and the ordinals across them run only here."""
    L = import_pkg("_lib")
    data = jpeg_cases.synthetic(768, 512, 77, quality=95, subsampling=0, restart_marker_rows=rows)
    groups = scan_bytes(data) * 8 // (L.RC_JPEG_ENTROPY_SUBSEQ_BITS * L.RC_JPEG_ENTROPY_GROUP_LANES)
    assert groups >= 3
    check_device_decoded(jpeg, dev, data)


def test_pixels_equal_the_host_stage(dev, host):
    datas = list(CASES.values())
    for a, b in zip(dev.decode(datas), host.decode(datas)):
        assert torch.equal(a, b)
    assert torch.equal(dev.decode_resized(datas, 224, 3), host.decode_resized(datas, 224, 3))


def mutations():
    """(name, bytes): damaged copies of the fixture and of the restart-marker stream."""
    out = []
    for src in ("test_image", "224_rst3"):
        data = CASES[src]
        sos = data.index(b"\xff\xda")
        first = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
        for cut in (1, 2, 4, 16):
            out.append((f"{src}_cut{cut}", data[:-cut]))
        out.append((f"{src}_cut_middle", data[:(first + len(data)) // 2]))
        rng = np.random.default_rng(len(data))
        for pos in rng.integers(first, len(data) - 2, 4):
            b = bytearray(data)
            b[pos] ^= 1 << int(rng.integers(0, 8))
            out.append((f"{src}_flip{pos}", bytes(b)))
        at = data.find(b"\xff\x00", first)
        if at >= 0:
            out.append((f"{src}_ff01", data[:at + 1] + b"\x01" + data[at + 2:]))
    rst = CASES["224_rst3"]
    m2, m5 = rst.index(b"\xff\xd2"), rst.index(b"\xff\xd5")
    out.append(("rst_removed", rst[:m2] + rst[m2 + 2:]))
    b = bytearray(rst)
    b[m2 + 1], b[m5 + 1] = b[m5 + 1], b[m2 + 1]
    out.append(("rst_swapped", bytes(b)))
    return out


def outcome(dec, data):
    try:
        return ("ok", dec.coefficients([data])[0])
    except Exception as e:  # the type and the message are what is compared
        return (type(e), str(e))


@pytest.mark.parametrize("name,data", mutations(), ids=[m[0] for m in mutations()])
def test_damaged_streams_get_the_hosts_verdict(jpeg, dev, host, name, data):
    if not jpeg.is_gpu_decodable(data):
        pytest.skip("the mutation left the header unsupported")
    got, want = outcome(dev, data), outcome(host, data)
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1]) if got[0] == "ok" else got[1] == want[1]
