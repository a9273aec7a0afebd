"""GPU PNG decode for the embedding path (replaces the PIL decode at
``embedding/main.py:97`` for non-interlaced 8-bit-or-less PNGs).

``probe(data)`` reads the header (size, depth, colour type, interlace, whether the GPU
path handles it); ``PngDecoder.decode(list_of_bytes)`` parses the chunks and inflates
IDAT on the host (``zlib`` in a small thread pool: it releases the GIL) and un-filters
and expands to HWC RGB u8 on the GPU (``rc_png_reconstruct``, one launch per batch),
or, with ``inflate="device"``, hands the compressed bytes to ``rc_png_decode``, whose
kernels inflate them into device memory (an image they refuse is inflated on the host,
with the host kind's result or error); either way
bit-exact with ``Image.open(...).convert("RGB")``: ``tRNS``, ``gAMA`` and ``iCCP`` are
ignored and alpha is dropped, as ``convert("RGB")`` does.  Streams the GPU path does not
handle (Adam7, 16-bit samples, APNG, rows wider than the kernel's carry row) are reported
by ``probe`` and by ``PngUnsupported``; damaged streams raise ``ValueError`` before any
library call.  The caller keeps both on the reference's host decode.
"""
from __future__ import annotations

import concurrent.futures as cf
import struct
import threading
import zlib
from typing import NamedTuple, Sequence

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8), 2: (8,), 3: (1, 2, 4, 8), 4: (8,), 6: (8,)}  # what the kernel reconstructs
MAX_UNITS = 3072  # widest row in filter units (csrc/png.hip: the carry row in LDS)
# Largest image the GPU path takes, in pixels.  Pillow guards the host decode against
# decompression bombs (it warns above Image.MAX_IMAGE_PIXELS = 89,478,485 and raises above twice
# that); a larger image is left to the host path so that guard decides as before.  The cap also
# bounds what one image may inflate to (4 bytes a pixel) and the library's staging.
MAX_PIXELS = 1 << 24
INFLATE_THREADS = 16
# Longest zlib stream the device inflate takes (RC_PNG_INFLATE_MAX_BYTES: its bit positions are
# int32); a longer one is inflated on the host.  No image of MAX_PIXELS pixels comes near it.
INFLATE_MAX_BYTES = 1 << 26
INFLATES = ("host", "device")


class PngUnsupported(ValueError):
    """A valid image the GPU decoder does not reconstruct (decode it on the host)."""


class PngInfo(NamedTuple):
    width: int
    height: int
    depth: int
    color: int
    interlace: int
    supported: int


def stride_of(width: int, depth: int, color: int) -> int:
    """Data bytes of one scanline (without its filter byte)."""
    return (width * depth * CHANNELS[color] + 7) // 8


def _chunks(data: bytes, verify: bool):
    """(type, body) of every chunk after the signature; ValueError on a cut or (verify) bad CRC."""
    if data[:8] != SIGNATURE:
        raise ValueError("not a PNG stream")
    at, n = 8, len(data)
    while at < n:
        if at + 8 > n:
            raise ValueError("PNG chunk header is cut short")
        (size,), kind = struct.unpack_from(">I", data, at), data[at + 4:at + 8]
        end = at + 12 + size
        if end > n:
            raise ValueError(f"PNG chunk {kind!r} is cut short")
        if verify and zlib.crc32(data[at + 4:end - 4]) != struct.unpack_from(">I", data, end - 4)[0]:
            raise ValueError(f"PNG chunk {kind!r} fails its CRC")
        yield kind, data[at + 8:end - 4]
        if kind == b"IEND":
            return
        at = end
    raise ValueError("PNG stream ends without IEND")


def _header(body: bytes, animated: bool) -> PngInfo:
    if len(body) != 13:
        raise ValueError("PNG IHDR is not 13 bytes")
    w, h, depth, color, comp, filt, lace = struct.unpack(">IIBBBBB", body)
    if w == 0 or h == 0 or color not in CHANNELS or depth not in (1, 2, 4, 8, 16) or comp or filt or lace > 1:
        raise ValueError("PNG IHDR holds a value the format does not allow")
    ok = (not lace and not animated and depth in DEPTHS[color] and w * h <= MAX_PIXELS
          and stride_of(w, depth, color) // max(1, depth * CHANNELS[color] // 8) <= MAX_UNITS)
    return PngInfo(w, h, depth, color, lace, int(ok))


def probe(data: bytes) -> PngInfo:
    """Header of a PNG stream; raises ValueError if ``data`` is not one.  Walks the chunk
    headers only (no CRC, no inflate): an ``acTL`` before ``IDAT`` marks an APNG."""
    it = _chunks(data, verify=False)
    kind, ihdr = next(it, (None, b""))
    if kind != b"IHDR":
        raise ValueError("PNG stream does not start with IHDR")
    animated = False
    for kind, _ in it:
        if kind == b"acTL":
            animated = True
        if kind in (b"acTL", b"IDAT"):
            break
    return _header(ihdr, animated)


def is_gpu_decodable(data: bytes) -> bool:
    if data[:8] != SIGNATURE:
        return False
    try:
        return bool(probe(data).supported)
    except ValueError:
        return False


class PngStream(NamedTuple):
    """An image whose IDAT is still compressed: what ``parse(data, inflate="device")`` returns."""
    info: PngInfo
    idat: bytes
    palette: "bytes | None"


def parse(data: bytes, inflate: str = "host"):
    """Full host stage of one image: (info, filtered scanlines, palette bytes or None).
    Every check the kernel's bounds rest on happens here; anything wrong is a ValueError.
    ``inflate="device"``: everything but the inflate (chunk walk, every CRC, the IHDR / PLTE
    rules, the two zlib header bytes) and a ``PngStream`` (info, joined IDAT bytes, palette); a
    stream above INFLATE_MAX_BYTES is inflated here as for "host"."""
    info, palette, idat, seen_idat, closed = None, None, [], False, False
    for kind, body in _chunks(data, verify=True):
        if info is None:
            if kind != b"IHDR":
                raise ValueError("PNG stream does not start with IHDR")
            info = _header(body, False)
        elif kind == b"IHDR":
            raise ValueError("PNG stream holds two IHDR chunks")
        elif kind in (b"acTL", b"fcTL", b"fdAT"):
            raise PngUnsupported("APNG stream: outside the GPU decoder's scope")
        elif kind == b"PLTE":
            if palette is not None or seen_idat or len(body) % 3 or not 3 <= len(body) <= 768:
                raise ValueError("PNG PLTE is misplaced or malformed")
            palette = body
        elif kind == b"IDAT":
            if closed:
                raise ValueError("PNG IDAT chunks are not consecutive")
            seen_idat = True
            idat.append(body)
        elif seen_idat:
            closed = True
    if info is None or not seen_idat:
        raise ValueError("PNG stream holds no image data")
    if not info.supported:
        raise PngUnsupported("PNG stream outside the GPU decoder's scope (interlaced, 16-bit, too wide or too large)")
    if info.color == 3 and palette is None:
        raise ValueError("indexed PNG without PLTE")
    palette = palette if info.color == 3 else None
    idat = idat[0] if len(idat) == 1 else b"".join(idat)
    if inflate == "device" and len(idat) <= INFLATE_MAX_BYTES:
        # CM = 8 (deflate), CINFO <= 7 (32 KiB window), FCHECK, FDICT = 0: what zlib checks first
        if len(idat) < 6 or idat[0] & 15 != 8 or idat[0] >> 4 > 7 or (idat[0] << 8 | idat[1]) % 31 or idat[1] & 32:
            raise ValueError("PNG IDAT does not inflate: bad zlib header")
        return PngStream(info, idat, palette)
    return info, inflate_idat(info, idat), palette


def inflate_idat(info: PngInfo, idat: bytes) -> bytes:
    """The host inflate of one image's joined IDAT bytes, with its checks: the filtered scanlines."""
    want = info.height * (1 + stride_of(info.width, info.depth, info.color))
    z = zlib.decompressobj()
    try:
        raw = z.decompress(idat, want + 1)  # one byte over: an over-long stream is seen, not inflated
    except zlib.error as e:
        raise ValueError(f"PNG IDAT does not inflate: {e}") from None
    if len(raw) != want or not z.eof:
        raise ValueError(f"PNG IDAT inflates to {len(raw)}{'' if z.eof else '+'} bytes, the header needs {want}")
    worst = max(raw[::want // info.height])
    if worst > 4:
        raise ValueError(f"PNG filter byte {worst} (0..4 exist)")
    # an index past PLTE is not an error for Pillow (it reads black), so it is none here either
    return raw


_pool = None
_pool_lock = threading.Lock()


def _inflate_pool() -> cf.ThreadPoolExecutor:
    global _pool
    with _pool_lock:
        if _pool is None:
            _pool = cf.ThreadPoolExecutor(INFLATE_THREADS, thread_name_prefix="png-inflate")
        return _pool


def stage(datas: Sequence[bytes], tolerant: bool = False, inflate: str = "host") -> list:
    """parse() of every image, inflating in the thread pool (one image: in the caller).  No device
    work.  ``tolerant``: an image that fails holds its ValueError in the list instead of raising."""
    def one(data):
        try:
            return parse(data, inflate)
        except ValueError as e:
            if not tolerant:
                raise
            return e

    return [one(datas[0])] if len(datas) == 1 else list(_inflate_pool().map(one, datas))


class PngDecoder:
    """Batched GPU PNG decoder: at most ``max_images`` images and ``max_pixels`` pixels per launch
    (a single image is at most MAX_PIXELS, whatever ``max_pixels`` says).  The library's staging
    grows with the largest launch, up to its own cap, and is reused."""

    def __init__(self, device=None, max_images: int = 256, max_pixels: int = 1 << 26, inflate: str = "host"):
        import torch

        from ._lib import load

        if inflate not in INFLATES:
            raise ValueError(f"inflate must be one of {INFLATES}, not {inflate!r}")
        self.inflate = inflate
        self.lib = load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   (device.index if isinstance(device, torch.device) else int(device)))
        self.max_images, self.max_pixels = int(max_images), int(max_pixels)

    def close(self) -> None:
        pass  # the staging belongs to the library (per device), not to this object

    host_stage = staticmethod(stage)

    def decode(self, datas: Sequence[bytes], stream=None) -> list:
        """PNG byte strings -> device u8 HWC RGB tensors (views into one buffer per chunk), input order."""
        return self.reconstruct(stage(datas, inflate=self.inflate), stream=stream)

    def _call(self, fn, *args):
        from ._lib import RC_ERR_UNSUPPORTED, check

        status = fn(*args)
        if status == RC_ERR_UNSUPPORTED:
            raise PngUnsupported(self.lib.rc_last_error().decode())
        check(status)

    def reconstruct(self, staged: Sequence, stream=None, tolerant: bool = False) -> list:
        """The device stage: host_stage()'s results -> device images.  Per chunk, the PngStream
        entries go through rc_png_decode (device inflate + reconstruction) and the inflated ones,
        with the streams the device flagged and the host then inflated, through one
        rc_png_reconstruct.  ``tolerant``: a flagged stream the host refuses too holds its
        ValueError in the list instead of raising."""
        import ctypes

        import torch

        from ._lib import PngImage, PngStream as CStream, stream_ptr

        pixels = [info.width * info.height for info, _, _ in staged]
        if pixels and max(pixels) > min(self.max_pixels, MAX_PIXELS):
            raise PngUnsupported(f"an image of {max(pixels)} pixels is above the decoder's limit")
        outs: list = []
        s = 0
        while s < len(staged):  # chunks of at most max_images images and max_pixels pixels
            e, px = s + 1, pixels[s]
            while e < len(staged) and e - s < self.max_images and px + pixels[e] <= self.max_pixels:
                px += pixels[e]
                e += 1
            chunk = list(staged[s:e])
            offs, off = [], 0
            for info, _, _ in chunk:
                offs.append(off)
                off += (info.width * info.height * 3 + 255) & ~255  # every image 256-byte aligned
            buf = torch.empty(off, dtype=torch.uint8, device=self.device)
            sp = stream_ptr(stream or torch.cuda.current_stream(self.device))

            def fill(rec, k, data_field, size_field):
                info, body, palette = chunk[k]
                rec.width, rec.height, rec.depth, rec.color = info.width, info.height, info.depth, info.color
                rec.palette_entries = len(palette) // 3 if palette else 0
                rec.palette, rec.out_offset = palette, offs[k]
                setattr(rec, data_field, body)
                setattr(rec, size_field, len(body))

            failed = {}
            dev = [k for k, item in enumerate(chunk) if isinstance(item, PngStream)]
            if dev:
                streams, flags = (CStream * len(dev))(), (ctypes.c_int32 * len(dev))()
                for rec, k in zip(streams, dev):
                    fill(rec, k, "idat", "idat_bytes")
                self._call(self.lib.rc_png_decode, self.device.index, len(dev), streams, buf.data_ptr(), off, flags, sp)
                for k, flagged in zip(dev, flags):
                    if flagged:  # the host inflates it, with the host kind's result or error
                        info, idat, palette = chunk[k]
                        try:
                            chunk[k] = (info, inflate_idat(info, idat), palette)
                        except ValueError as err:
                            if not tolerant:
                                raise
                            failed[k] = err
            host = [k for k, item in enumerate(chunk) if not isinstance(item, PngStream)]
            if host:
                images = (PngImage * len(host))()
                for rec, k in zip(images, host):
                    fill(rec, k, "scanlines", "scan_bytes")
                self._call(self.lib.rc_png_reconstruct, self.device.index, len(host), images, buf.data_ptr(), off, sp)
            for k, (info, _, _) in enumerate(chunk):
                outs.append(failed.get(k, None) or
                            buf[offs[k]:offs[k] + info.width * info.height * 3].view(info.height, info.width, 3))
            s = e
        return outs


__all__ = ["PngDecoder", "PngInfo", "PngStream", "PngUnsupported", "probe", "is_gpu_decodable", "parse", "inflate_idat",
           "stage"]
