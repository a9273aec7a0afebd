"""GPU PNG decode (host inflate + rc_png_reconstruct) against Pillow's decode of the same bytes,
``Image.open(BytesIO(png)).convert("RGB")`` — the reference's own path, embedding/main.py:97.
Integer work: exact equality.  The streams are built here so that every filter type is forced."""
import struct
import zlib
from io import BytesIO

import numpy as np
import pytest
from PIL import Image

from conftest import import_pkg

pytestmark = pytest.mark.gpu

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
TYPES = [(0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (6, 8)]
SHAPES = [(1, 1), (3, 2), (63, 65), (64, 64), (65, 129), (300, 168)]


def chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def make_png(w, h, color, depth, filt, seed=0) -> bytes:
    """A PNG of uniform random scanline bytes, row r filtered with ``filt`` (0..4, or r % 5 for
    "cycling").  An indexed image gets a PLTE one entry short of 2**depth (200 at depth 8), so
    some indices lie past it."""
    rng = np.random.default_rng([seed, w, h, color, depth])
    bits = depth * CHANNELS[color]
    stride, bpp = (w * bits + 7) // 8, max(1, bits // 8)
    rows = rng.integers(0, 256, (h, stride)).astype(np.int32)
    left = lambda v: np.concatenate([np.zeros(bpp, np.int32), v[:-bpp]])
    raw = bytearray()
    for r in range(h):
        f = r % 5 if filt == "cycling" else filt
        x, b = rows[r], rows[r - 1] if r else np.zeros(stride, np.int32)
        a, c = left(x), left(b)
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        raw += bytes([f]) + ((x - [0 * a, a, b, (a + b) // 2, paeth][f]) & 255).astype(np.uint8).tobytes()
    plte = chunk(b"PLTE", rng.integers(0, 256, 3 * min(200, 2 ** depth - 1), dtype=np.uint8).tobytes()) if color == 3 else b""
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color, 0, 0, 0)) + plte
            + chunk(b"IDAT", zlib.compress(bytes(raw), 1)) + chunk(b"IEND", b""))


def pil_rgb(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(BytesIO(data)).convert("RGB"))


@pytest.fixture(scope="module")
def dec(cuda):
    return import_pkg("png").PngDecoder(device=0)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4, "cycling"])
@pytest.mark.parametrize("color,depth", TYPES)
def test_parity_with_pillow(dec, color, depth, filt, shape):
    data = make_png(shape[0], shape[1], color, depth, filt)
    (got,) = dec.decode([data])
    assert np.array_equal(got.cpu().numpy(), pil_rgb(data))


def test_mixed_batch_keeps_order_and_reuses_the_workspace(dec):
    b = BytesIO()
    Image.fromarray(np.random.default_rng(3).integers(0, 256, (77, 130, 3), dtype=np.uint8)).save(b, format="PNG")
    datas = [make_png(300, 168, 2, 8, "cycling", 1), make_png(9, 70, 3, 2, 4), b.getvalue(), make_png(1, 1, 0, 1, 0),
             make_png(200, 131, 6, 8, 4), make_png(65, 129, 4, 8, 3), make_png(130, 3, 0, 4, "cycling")]
    refs = [pil_rgb(d) for d in datas]
    lib = import_pkg("_lib").load()
    for call in range(2):
        n0 = lib.rc_alloc_count()
        outs = dec.decode(datas)
        assert [tuple(o.shape) for o in outs] == [r.shape for r in refs]
        for o, r in zip(outs, refs):
            assert np.array_equal(o.cpu().numpy(), r)
    assert lib.rc_alloc_count() == n0  # the second call staged into the first one's blocks


def test_decode_many_serves_pngs_from_the_device(cuda, monkeypatch):
    """An interleaved JPEG / PNG list through the services' decode: the PNGs come back as device
    tensors, and the embeddings equal those of the host PNG decode (RC_GPU_PNG=0) bit for bit."""
    import torch

    main = import_pkg("embedding.main")
    rng = np.random.default_rng(5)
    blobs = []
    for i, (w, h) in enumerate([(300, 168), (224, 224), (300, 168), (61, 200)]):
        b = BytesIO()
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(b, format="JPEG" if i == 1 else "PNG")
        blobs.append(b.getvalue())
    blobs.append(make_png(300, 168, 3, 4, "cycling"))
    monkeypatch.setattr(main.Config, "GPU_PNG", True)
    images = main.decode_many(blobs)
    assert all(isinstance(im, torch.Tensor) and im.is_cuda for im in images)
    for i in (0, 2, 3, 4):
        assert np.array_equal(images[i].cpu().numpy(), pil_rgb(blobs[i]))
    # one byte more than the header needs: Pillow takes it, the parser does not; only that blob
    # goes to the host, the others still come from the device
    lenient = (blobs[4][:8] + chunk(b"IHDR", struct.pack(">IIBBBBB", 1, 1, 8, 2, 0, 0, 0))
               + chunk(b"IDAT", zlib.compress(b"\x00abcd")) + chunk(b"IEND", b""))
    mixed = main.decode_many(blobs[:3] + [lenient] + blobs[3:])
    assert isinstance(mixed[3], np.ndarray) and np.array_equal(mixed[3], pil_rgb(lenient))
    assert all(isinstance(im, torch.Tensor) for k, im in enumerate(mixed) if k != 3)
    raw_gpu, _ = main.embed_many_device(blobs)
    monkeypatch.setattr(main.Config, "GPU_PNG", False)
    assert not any(isinstance(main.decode_many(blobs)[i], torch.Tensor) for i in (0, 2, 3, 4))
    raw_host, _ = main.embed_many_device(blobs)
    assert torch.equal(raw_gpu, raw_host)
