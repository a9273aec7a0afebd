"""PngDecoder(inflate="device"): the token-parallel DEFLATE kernels (csrc/png_inflate.hip) against
Pillow's decode of the same bytes, exact equality, with rc_png_decode_stats showing that the
device and not the host fallback produced every valid image.  The streams are the smallest at
which each mechanism can go wrong; the three "window" shapes are derived from the kernel's split
(LANES lanes of ROW_BITS bits: a window of 32,768 bits).  The damaged streams check the verdict
only (the same exception type or the same pixels as inflate="host"); each of them, like every
valid case, went through tools/inflate_check (the same decoder core, serial, built with
-fsanitize=address,undefined) before it went to a GPU."""
import struct
import zlib
from io import BytesIO

import numpy as np
import pytest
from PIL import Image

from conftest import import_pkg

pytestmark = pytest.mark.gpu

ROW_BITS, LANES = 128, 256  # RC_PNG_INFLATE_ROW_BITS, RC_PNG_INFLATE_LANES (asserted below)
WINDOW = ROW_BITS * LANES


def chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def wrap(z: bytes, w: int, h: int, color: int, split=None) -> bytes:
    """A PNG around the zlib stream ``z``; ``split``: the sizes of the first IDAT chunks."""
    cuts = np.cumsum([0] + list(split or []))
    parts = [z[a:b] for a, b in zip(cuts, cuts[1:])] + [z[cuts[-1]:]]
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color, 0, 0, 0))
            + b"".join(chunk(b"IDAT", p) for p in parts) + chunk(b"IEND", b""))


def deflate(a: np.ndarray, level=9, strategy=zlib.Z_DEFAULT_STRATEGY, flush_rows=False, empty_final=False, filt=0) -> bytes:
    """zlib stream of the image's scanlines, every row with filter byte ``filt`` (0: None)."""
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    out = b""
    for row in a.reshape(a.shape[0], -1):
        out += co.compress(bytes([filt]) + row.tobytes())
        if flush_rows:
            out += co.flush(zlib.Z_FULL_FLUSH)  # ends the block and appends an empty stored one
    if empty_final and not flush_rows:
        out += co.flush(zlib.Z_FULL_FLUSH)
    return out + co.flush()


def png(a: np.ndarray, split=None, **kw) -> bytes:
    return wrap(deflate(a, **kw), a.shape[1], a.shape[0], 2 if a.ndim == 3 else 0, split)


def literal_block(h: int, w: int, long_codes: int) -> bytes:
    """A gray image that Z_FIXED codes as ONE block of literals only: no byte pair occurs twice in
    the data, so no match exists; values below 144 take 8 bits and ``long_codes`` values of 200+
    take 9.  The block's tokens are then 8 h (w + 1) + long_codes + 7 bits, which is checked."""
    seq = [v for a in range(1, 92) for b in range(a + 1, 92) for v in (a, b)][:h * w]
    a = np.array(seq, dtype=np.uint8).reshape(h, w)
    a[0, :long_codes] = np.arange(200, 200 + long_codes)
    data = png(a, level=9, strategy=zlib.Z_FIXED)
    bits = 3 + 8 * h * (w + 1) + long_codes + 7
    assert len(deflate(a, strategy=zlib.Z_FIXED)) == 2 + (bits + 7) // 8 + 4
    return data


def by_hand(head: bytes, tokens: str, raw: bytes, w: int, h: int) -> bytes:
    """A gray PNG whose stream is written out: ``head`` (whole bytes after the zlib header), then a
    final fixed block of ``tokens`` ('0' / '1' in stream order) and end-of-block; ``raw``: what it
    inflates to."""
    bits = "1" + "10" + tokens + "0000000"
    block = int(bits[::-1], 2).to_bytes((len(bits) + 7) // 8, "little")
    return wrap(b"\x78\x01" + head + block + struct.pack(">I", zlib.adler32(raw)), w, h, 0)


def far_match(stored: int) -> bytes:
    """1023 x 64: one stored block of ``stored`` bytes (32,768: 32 noise rows) and a fixed block of
    128 matches of length 256 at distance 32,768, the largest there is.  With ``stored`` one less,
    the first match reaches one byte before the start of the data."""
    rows = np.random.default_rng(11).integers(0, 256, (32, 1023), dtype=np.uint8)
    raw = b"".join(b"\x00" + r.tobytes() for r in rows)
    match = "11000100" + "10111" + "11101" + "1" * 13  # symbol 284 + 29: 256; symbol 29 + 8191: 32,768
    return by_hand(b"\x00" + struct.pack("<HH", stored, stored ^ 0xFFFF) + raw[:stored], match * 128, raw + raw, 1023, 64)


def match_across_the_window(k: int) -> bytes:
    """682 x 6: (WINDOW - k) / 8 literals of 8 bits, then a match of 12 bits (length 3, distance 1)
    that starts k bits before the first window's end and ends in the second."""
    n = (WINDOW - k) // 8
    raw = bytes((7 * i + 3) % 144 if i % 683 else 0 for i in range(n))
    assert n + 3 == 6 * 683 and k < 12
    return by_hand(b"", "".join(format(0x30 + v, "08b") for v in raw) + "0000001" + "00000", raw + raw[-1:] * 3, 682, 6)


def longest_literal_code(z: bytes) -> int:
    """The longest literal code of the stream's first block, which must be a dynamic one."""
    bits, at = int.from_bytes(z[2:600], "little"), 0

    def take(k):
        nonlocal at
        at += k
        return bits >> (at - k) & ((1 << k) - 1)

    assert take(1) in (0, 1) and take(2) == 2, "not a dynamic block"
    hlit, _, hclen = take(5) + 257, take(5), take(4) + 4
    cl = dict(zip([16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15], [take(3) for _ in range(hclen)]))
    codes, code, lens = {}, 0, []
    for n in range(1, 8):  # the code-length alphabet's canonical codes
        for sym in sorted(k for k, v in cl.items() if v == n):
            codes[n, code] = sym
            code += 1
        code <<= 1
    while len(lens) < hlit:
        n = code = 0
        while (n, code) not in codes:
            n, code = n + 1, code << 1 | take(1)
        sym = codes[n, code]
        lens += [sym] if sym < 16 else [lens[-1]] * (3 + take(2)) if sym == 16 else [0] * (3 + take(3) if sym == 17 else 11 + take(7))
    return max(lens[:256])


def smooth(w: int, h: int) -> np.ndarray:
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    return np.stack([127 + 90 * np.sin(x / (11 + 9 * c)) * np.cos(y / (17 + 5 * c)) for c in range(3)], -1).astype(np.uint8)


def saved(a: np.ndarray) -> bytes:
    b = BytesIO()
    Image.fromarray(a).save(b, format="PNG")
    return b.getvalue()


RNG = np.random.default_rng(7)
NOISE = RNG.integers(0, 256, (168, 300, 3), dtype=np.uint8)
SKEWED = np.minimum(RNG.geometric(0.06, (168, 300, 3)) - 1, 255).astype(np.uint8)  # rare values: long codes
SMALL = smooth(40, 24)
TILE = np.tile(RNG.integers(0, 256, (31, 1047), dtype=np.uint8), (3, 1))  # rows repeat 32,488 bytes on
CASES = {
    "stored": png(SMALL, level=0),
    "fixed": png(SMALL, strategy=zlib.Z_FIXED),
    "dynamic": png(SMALL),
    "blocks_per_row": png(SMALL, flush_rows=True),        # a block and an empty stored block per row
    "empty_final_block": png(SMALL, empty_final=True),
    "one_pixel": png(np.full((1, 1, 3), 77, np.uint8)),
    "shorter_than_a_row": literal_block(1, 13, 0),        # 119 token bits < ROW_BITS
    "one_window_exactly": literal_block(63, 64, 1),       # WINDOW token bits: end-of-block ends lane 255's row
    "one_window_and_a_bit": literal_block(63, 64, 2),     # WINDOW + 1: it ends in the overhang
    "end_of_block_opens_a_window": literal_block(64, 63, 0),  # WINDOW + 7: it starts the second window
    "constant": png(np.zeros((168, 300, 3), np.uint8)),   # distance 1, length 258: self-overlapping copies
    "far_rows": png(TILE),                                # matches near zlib's largest distance (32,506)
    "distance_32768": far_match(32768),
    "match_across_windows": match_across_the_window(8),
    "crosses_windows": saved(smooth(300, 168)),           # ten windows, filtered rows, many matches
    "split_idat": png(SMALL, split=[1, 1, 7, 40]),
    "noise": png(NOISE),                                  # uniform noise: zlib stores it, five stored blocks
    # skewed noise, Huffman only: dynamic blocks of literals over some twenty windows, codes above the lookahead
    "long_codes": png(SKEWED, strategy=zlib.Z_HUFFMAN_ONLY),
}
assert longest_literal_code(deflate(SKEWED, strategy=zlib.Z_HUFFMAN_ONLY)) > 10  # kLitLook
BATCH = ["dynamic", "stored", "long_codes", "one_pixel", "constant", "split_idat", "one_window_and_a_bit", "crosses_windows"]


def poked(data: bytes, at: int, value: int) -> bytes:
    """``data`` with byte ``at`` of its (single) IDAT body replaced, the chunk's CRC recomputed."""
    i = data.index(b"IDAT")
    (n,) = struct.unpack_from(">I", data, i - 4)
    z = bytearray(data[i + 4:i + 4 + n])
    z[at] = value
    return data[:i - 4] + chunk(b"IDAT", bytes(z)) + data[i + 8 + n:]


def rebody(data: bytes, edit) -> bytes:
    i = data.index(b"IDAT")
    (n,) = struct.unpack_from(">I", data, i - 4)
    return data[:i - 4] + chunk(b"IDAT", edit(data[i + 4:i + 4 + n])) + data[i + 8 + n:]


BASE = CASES["dynamic"]  # byte 2 of its stream holds BFINAL, BTYPE and HLIT; bytes 3.. the code-length set
DAMAGED = {
    "btype_3": poked(BASE, 2, 0x07),
    "code_length_set_oversubscribed": poked(BASE, 5, 0x49),
    "code_length_set_poke_1": poked(BASE, 6, 0x92),
    "code_length_set_poke_2": poked(BASE, 7, 0x24),
    "repeat_without_previous": poked(BASE, 12, 0x00),
    "lengths_poke_1": poked(BASE, 14, 0xFF),
    "lengths_poke_2": poked(BASE, 20, 0x00),
    "hlit_poke": poked(BASE, 2, 0xFD),
    "token_poke_1": poked(BASE, 60, 0xFF),
    "token_poke_2": poked(BASE, 90, 0x00),
    "token_poke_3": poked(BASE, 120, 0xA5),
    "distance_past_the_start": far_match(32767),
    "truncated_in_tokens": rebody(BASE, lambda z: z[:len(z) // 2]),
    "truncated_in_header": rebody(BASE, lambda z: z[:9]),
    "truncated_in_adler": rebody(BASE, lambda z: z[:-2]),
    "one_extra_byte": rebody(BASE, lambda z: z + b"\x00"),
    "wrong_adler": rebody(BASE, lambda z: z[:-1] + bytes([z[-1] ^ 1])),
    "filter_byte_5": png(SMALL, filt=5),
    "stored_len_not_nlen": poked(CASES["stored"], 5, 0x00),
    "one_row_short": wrap(deflate(SMALL[:-1]), 40, 24, 2),
    "one_row_long": wrap(deflate(smooth(40, 25)), 40, 24, 2),
}


def pil_rgb(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(BytesIO(data)).convert("RGB"))


@pytest.fixture(scope="module")
def lib(cuda):
    L = import_pkg("_lib")
    assert (L.RC_PNG_INFLATE_ROW_BITS, L.RC_PNG_INFLATE_LANES) == (ROW_BITS, LANES)
    return L.load()


@pytest.fixture(scope="module")
def dec(lib):
    return import_pkg("png").PngDecoder(device=0, inflate="device")


def stats(lib):
    import ctypes

    a, b = ctypes.c_int64(), ctypes.c_int64()
    assert lib.rc_png_decode_stats(0, ctypes.byref(a), ctypes.byref(b)) == 0
    return a.value, b.value


@pytest.mark.parametrize("name", list(CASES))
def test_device_inflate_equals_pillow_without_fallback(lib, dec, name):
    before = stats(lib)
    (got,) = dec.decode([CASES[name]])
    assert np.array_equal(got.cpu().numpy(), pil_rgb(CASES[name]))
    after = stats(lib)
    assert (after[0] - before[0], after[1] - before[1]) == (1, 0)


def test_mixed_batch_keeps_order_and_reuses_the_workspace(lib, dec):
    datas = [CASES[k] for k in BATCH]
    for call in range(2):
        n0, before = lib.rc_alloc_count(), stats(lib)
        outs = dec.decode(datas)
        for o, d in zip(outs, datas):
            assert np.array_equal(o.cpu().numpy(), pil_rgb(d))
        assert stats(lib) == (before[0] + len(datas), before[1])
    assert lib.rc_alloc_count() == n0  # the second call staged into the first one's blocks


def test_both_kinds_in_one_chunk_share_the_buffer(lib, dec):
    """Host-inflated and compressed entries interleaved in one reconstruct(): rc_png_decode's images
    and rc_png_reconstruct's land at their own offsets of the chunk's buffer, in input order.  This
    is the path a flagged image takes once the host has inflated it."""
    png_mod = import_pkg("png")
    datas = [CASES[k] for k in BATCH]
    staged = [png_mod.parse(d, inflate="device" if k % 2 else "host") for k, d in enumerate(datas)]
    before = stats(lib)
    for o, d in zip(dec.reconstruct(staged), datas):
        assert np.array_equal(o.cpu().numpy(), pil_rgb(d))
    assert stats(lib) == (before[0] + len(datas) // 2, before[1])


@pytest.mark.parametrize("name", list(DAMAGED))
def test_damaged_stream_gets_the_host_kinds_verdict(lib, dec, name):
    host = import_pkg("png").PngDecoder(device=0)

    def outcome(d):
        try:
            return d.decode([CASES["fixed"], DAMAGED[name]])[1].cpu().numpy()
        except ValueError as e:
            return type(e)

    want, got = outcome(host), outcome(dec)
    assert (want is got) if isinstance(want, type) else np.array_equal(want, got)


def test_service_path_embeds_the_same_bits(cuda, monkeypatch):
    """RC_GPU_INFLATE through decode_many + embed: two PNGs and a JPEG, embeddings bit-equal to the
    default path's, and the PNGs inflated by the device."""
    import torch

    main = import_pkg("embedding.main")
    lib = import_pkg("_lib").load()
    b = BytesIO()
    Image.fromarray(NOISE).save(b, format="JPEG")
    blobs = [CASES["crosses_windows"], b.getvalue(), CASES["long_codes"]]
    raw_host, _ = main.embed_many_device(blobs)
    monkeypatch.setattr(main.Config, "GPU_INFLATE", True)
    main.reset_embedder()
    try:
        before = stats(lib)
        raw_dev, _ = main.embed_many_device(blobs)
        assert stats(lib) == (before[0] + 2, before[1])
    finally:
        main.reset_embedder()
    assert torch.equal(raw_dev, raw_host)
