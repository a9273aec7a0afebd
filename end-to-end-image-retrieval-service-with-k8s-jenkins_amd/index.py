"""In-HBM exact cosine index behind Pinecone's ``Index`` shape.

Replaces the remote Pinecone index the reference opens in ``get_index``
(``ingesting/utils.py:23-38`` = ``retriever/utils.py:23-38``) and calls at
``index.upsert([(id, feature, metadata)])`` (``ingesting/main.py:156-158``),
``index.query(vector=..., top_k=..., include_values=True)["matches"]``
(``retriever/utils.py:62-64``) and ``index.fetch(ids=...)``
(``retriever/main.py:142``, consumed at ``:151-153``).

Split of work: string ids, metadata and the id → row map stay on the host
(Pinecone ids are uuid4 strings, ``ingesting/main.py:127``); the device holds
only the L2-normalised rows, written and searched by the HIP library through
the C ABI (``include/retrieval_core.h``).
"""
from __future__ import annotations

import array
import json
import os
import threading
from typing import Any, Iterable, Sequence

import numpy as np
import torch

from . import _lib, compaction, metacolumns, metafilter, pages, sparsevalues
from ._lib import check, ptr, stream_ptr

# query_batch(filter=..., mode="auto") takes the batched MFMA path when the unmasked conditions
# hold AND at least this share of the rows is eligible.  Ineligible rows still pass the filter
# GEMM and take candidate slots (the threshold only rises with eligible rows), so candidates per
# stage grow by 1 / share and overflow into the exact fallback scan below a share of about
# 0.37 (k = 100).  Measured on an MI355X (tools/masked_search_micro.py; DESIGN.md, "Masked
# search"; 1M x 512 f16, 256 queries x top-100): MFMA is 23x faster than the masked scan at
# share 0.5 with no fallback, level with it at 0.1 (every query falls back) and 4.8x slower at
# 0.01.  0.5 is the lowest measured share at which MFMA wins without falling back.
MASKED_MFMA_MIN_SHARE = 0.5
# Below that share "auto" asks for "mfma_masked" (the mask inside the filter GEMM: candidates per
# stage no longer grow with 1 / share) inside the box that was measured, and scans outside it.
# Source: tools/masked_search_micro.py --part maskfilter on an MI355X (records appended to
# profiles/masked_search/masked_search_micro.jsonl; DESIGN.md, "Masked search"): "mfma_masked"
# against the masked scan, f16 x 512, uniformly random masks at shares 0.25 / 0.1 / 0.01 / 0.001,
# top-10 and top-100, 16 / 32 / 64 / 256 queries over 65,536 and 1M rows, 32 / 256 queries over 16M.
# The bar is 2x, not 1x: the host does not know how clustered a mask is, a clustered mask makes the
# scan up to 2x cheaper at equal share, and it saves the filter GEMM nothing.
#   MASK_FILTER_MIN_QUERIES  up to 1M rows every measured cell from 32 queries on is at least 3.16x
#       ahead (the lowest: 32 x top-100 at share 0.25 over 65,536 rows).  At 16 queries the cells lie
#       between 1.98x and 4.08x, one under the bar and four within 10 % of it: 16-31 queries scan.
#   MASK_FILTER_MIN_SHARE    the most selective share measured; below it nothing was measured.
#   MASK_FILTER_MIN_ROWS / MASK_FILTER_MAX_ROWS  the smallest and largest measured rows per shard
#       (the smallest is also the unmasked "auto" bound); larger shards scan until they are measured.
#   MASK_FILTER_LARGE_ROWS, MASK_FILTER_LARGE_MIN_QUERIES, MASK_FILTER_LARGE_MIN_SHARE  the filter
#       GEMM reads every row whatever the share, while the masked scan skips 8-row groups without an
#       eligible row, so over many rows a very selective mask favours the scan: over 16M rows 32
#       queries are 6.5x-17x ahead at shares 0.25 and 0.1, but 1.9x-2.3x at 0.01 and level at 0.001;
#       256 queries stay at least 6.26x ahead down to 0.001.  Above 1M rows per shard (the largest
#       size whose every cell from 32 queries clears the bar) the rule therefore wants 256 queries
#       or a share of at least 0.1; 64 queries were not measured over 16M rows and count as 32.
# k does not enter: top-10 and top-100 were measured in every cell, and the rule holds for both.
MASK_FILTER_MIN_QUERIES = 32
MASK_FILTER_MIN_SHARE = 0.001
MASK_FILTER_MIN_ROWS = 65536
MASK_FILTER_MAX_ROWS = 16_000_000
MASK_FILTER_LARGE_ROWS = 1_000_000
MASK_FILTER_LARGE_MIN_QUERIES = 256
MASK_FILTER_LARGE_MIN_SHARE = 0.1
BITMAP_CACHE_ENTRIES = 8


def _device_index(device) -> int:
    if device is None:
        return torch.cuda.current_device()
    if isinstance(device, torch.device):
        return device.index if device.index is not None else torch.cuda.current_device()
    if isinstance(device, str):
        d = torch.device(device)
        return d.index if d.index is not None else torch.cuda.current_device()
    return int(device)


class DeviceIndex:
    """One ``rc_index`` handle: a block of row slots on one GPU (a shard).

    A search returns ``row_base + local_row * row_stride`` (``set_row_map``):
    the global rows of a round-robin shard."""

    def __init__(self, dim: int, dtype: str = "float32", capacity: int = 1 << 20, device=None, row_base: int = 0,
                 row_stride: int = 1, _handle=None, metric: str = "cosine"):
        self.lib = _lib.load()
        if dtype not in _lib.DTYPES:
            raise ValueError(f"unknown index dtype {dtype!r}")
        if metric not in _lib.METRICS:
            raise ValueError(f"unknown metric {metric!r} (expected one of {sorted(_lib.METRICS)})")
        self.dim = int(dim)
        self.dtype = dtype
        self.device_index = _device_index(device)
        self.device = torch.device("cuda", self.device_index)
        self.row_base = int(row_base)
        self.row_stride = int(row_stride)
        self._owned = _handle is None
        if _handle is None:
            h = _lib.C.c_void_p()
            check(self.lib.rc_index_create(self.device_index, self.dim, _lib.DTYPES[dtype], int(capacity), self.row_base,
                                           _lib.C.byref(h)))
            self._h = h
            if self.row_stride != 1:
                self.set_row_map(self.row_base, self.row_stride)
            if metric != "cosine":
                self.set_metric(metric)
        else:  # a shard borrowed from an rc_sharded handle (owned there, its metric set there)
            self._h = _handle

    @property
    def handle(self):
        if self._h is None:
            raise RuntimeError("index is closed")
        return self._h

    @property
    def capacity(self) -> int:
        cap = _lib.C.c_int64()
        check(self.lib.rc_index_info(self.handle, None, None, _lib.C.byref(cap), None))
        return cap.value

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            if self._owned:
                check(self.lib.rc_index_destroy(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ld(self) -> int:
        ld = _lib.C.c_int64()
        check(self.lib.rc_index_info(self.handle, None, None, None, _lib.C.byref(ld)))
        return ld.value

    def set_row_map(self, row_base: int, row_stride: int = 1) -> None:
        check(self.lib.rc_index_set_row_map(self.handle, int(row_base), int(row_stride)))
        self.row_base, self.row_stride = int(row_base), int(row_stride)

    def grow(self, new_capacity: int, stream=None) -> None:
        check(self.lib.rc_index_grow(self.handle, int(new_capacity), stream_ptr(stream)))

    def reserve(self, max_nq: int, max_k: int) -> None:
        check(self.lib.rc_index_reserve(self.handle, int(max_nq), int(max_k)))

    def set_filter(self, kind: str, stream=None) -> None:
        """Filter kind of the batched search (rc_index_set_filter): "native" (the filter GEMM
        reads the stored f16/bf16 rows), "i8" (an int8 copy of every row, int8 MFMA at twice the
        f16 rate), "f8" (a float8 index only: the block-scaled fp8 MFMA on the stored rows, no
        copy; it is what gives a float8 index ``mode="mfma"``) or "metric" (an f16/bf16 index
        only: "native" under cosine, and under dotproduct / euclidean the same filter GEMM with
        a bound on the metric's own score, which is what gives a non-cosine index
        ``mode="mfma"``; no copy).  "i8" and "f8" are cosine-only.  Results never change —
        candidates are rescored exactly on the stored rows."""
        if kind not in _lib.FILTERS:
            raise ValueError(f"unknown filter {kind!r} (expected one of {sorted(_lib.FILTERS)})")
        check(self.lib.rc_index_set_filter(self.handle, _lib.FILTERS[kind], stream_ptr(stream)))

    @property
    def filter(self) -> str:
        k = _lib.C.c_int()
        check(self.lib.rc_index_get_filter(self.handle, _lib.C.byref(k)))
        return {v: n for n, v in _lib.FILTERS.items()}[k.value]

    def filter_scores(self, queries: torch.Tensor, row0: int, n: int, stream=None):
        """What the "f8" filter computes (rc_index_filter_scores): its scores ``s'`` of the
        queries against local rows [row0, row0 + n) (``row0`` a multiple of 128), f32 [nq, n],
        and each query's bound ``eps`` on ``|s' - exact score|``, f32 [nq].  Raises unless the
        filter kind is "f8"."""
        q = self._vecs(queries)
        out = torch.empty((q.shape[0], int(n)), dtype=torch.float32, device=self.device)
        eps = torch.empty((q.shape[0],), dtype=torch.float32, device=self.device)
        check(self.lib.rc_index_filter_scores(self.handle, ptr(q), q.shape[0], int(row0), int(n), ptr(out), ptr(eps),
                                              stream_ptr(stream)))
        return out, eps

    def set_metric(self, metric: str) -> None:
        """Scoring rule of the later searches (rc_index_set_metric): "cosine", "dotproduct" or
        "euclidean".  Touches no stored data, so it is legal on a populated index.  ``search``
        returns scores descending under every metric: Euclidean ones are ``-||q - v||^2``."""
        if metric not in _lib.METRICS:
            raise ValueError(f"unknown metric {metric!r} (expected one of {sorted(_lib.METRICS)})")
        check(self.lib.rc_index_set_metric(self.handle, _lib.METRICS[metric]))

    @property
    def metric(self) -> str:
        m = _lib.C.c_int()
        check(self.lib.rc_index_get_metric(self.handle, _lib.C.byref(m)))
        return {v: n for n, v in _lib.METRICS.items()}[m.value]

    def _vecs(self, vecs: torch.Tensor) -> torch.Tensor:
        if vecs.dim() == 1:
            vecs = vecs[None]
        if vecs.shape[-1] != self.dim:
            raise ValueError(f"Vector dimension {vecs.shape[-1]} does not match the dimension of the index {self.dim}")
        return vecs.to(device=self.device, dtype=torch.float32).contiguous()

    def upsert_rows(self, vecs: torch.Tensor, rows: torch.Tensor, stream=None) -> None:
        """rows must be distinct (rc_index_upsert); callers with repeated ids dedupe first."""
        vecs = self._vecs(vecs)
        rows = rows.to(device=self.device, dtype=torch.int64).contiguous()
        if rows.numel() != vecs.shape[0]:
            raise ValueError("rows and vectors differ in length")
        check(self.lib.rc_index_upsert(self.handle, ptr(vecs), vecs.shape[0], ptr(rows), stream_ptr(stream)))

    def move_rows(self, src, dst, stream=None) -> None:
        """Stored row dst[i] becomes a bit-for-bit copy of stored row src[i], norm included
        (rc_index_move_rows).  The two lists must be disjoint and dst must hold no row twice."""
        src = torch.as_tensor(src, dtype=torch.int64).to(self.device).contiguous()
        dst = torch.as_tensor(dst, dtype=torch.int64).to(self.device).contiguous()
        if src.numel() != dst.numel():
            raise ValueError("src and dst differ in length")
        check(self.lib.rc_index_move_rows(self.handle, ptr(src), ptr(dst), src.numel(), stream_ptr(stream)))

    def fetch_rows(self, rows: torch.Tensor, stream=None) -> torch.Tensor:
        rows = rows.to(device=self.device, dtype=torch.int64).contiguous()
        out = torch.empty((rows.numel(), self.dim), dtype=torch.float32, device=self.device)
        check(self.lib.rc_index_fetch(self.handle, ptr(rows), rows.numel(), ptr(out), stream_ptr(stream)))
        return out

    def search(self, queries: torch.Tensor, k: int, n_rows: int, stream=None, out=None, mode: str = "auto", mask=None):
        """Exact top-k over rows [0, n_rows) by the index's metric (cosine unless ``set_metric``
        said otherwise): (scores f32 [nq,k] descending, global rows i64 [nq,k]).

        ``mode``: "scan" (HBM-bound streaming scan), "mfma" (batched filter GEMM +
        exact rescoring, f16/bf16 index; under dotproduct / euclidean only with the "metric"
        filter) or "auto" (MFMA for >= 8 queries; a float8 index scans and refuses "mfma" unless
        its filter is "f8", a non-cosine index unless its filter is "metric").
        ``mask``: optional row-eligibility bitmap over the LOCAL rows (rc_index_search_masked):
        an int32 / uint32 tensor of ceil(n_rows / 32) words on this device, bit r & 31 of word
        r >> 5 = row r may be returned; "auto" then scans.  "mfma" with a mask keeps the filter
        GEMM as it is and drops ineligible candidates when rescoring (fast while at least half
        of the rows are eligible); "mfma_masked" applies the mask inside the filter GEMM as
        well, so a selective mask no longer overflows the candidate lists.  It is refused
        where "mfma" is, and without a mask it is "mfma"."""
        if mode not in _lib.SEARCH_MODES:
            raise ValueError(f"unknown search mode {mode!r}")
        q = self._vecs(queries)
        nq = q.shape[0]
        if out is None:
            scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
            rows = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        else:
            scores, rows = out
        if mask is None:
            check(self.lib.rc_index_search_ex(self.handle, ptr(q), nq, int(n_rows), int(k), ptr(scores), ptr(rows),
                                              _lib.SEARCH_MODES[mode], stream_ptr(stream)))
            return scores, rows
        if mask.dtype not in (torch.int32, torch.uint32) or mask.numel() < (int(n_rows) + 31) // 32:
            raise ValueError("mask must hold ceil(n_rows / 32) 32-bit words")
        mask = mask.to(device=self.device).contiguous()
        check(self.lib.rc_index_search_masked(self.handle, ptr(q), nq, int(n_rows), int(k), ptr(mask), ptr(scores),
                                              ptr(rows), _lib.SEARCH_MODES[mode], stream_ptr(stream)))
        return scores, rows

    def set_pages(self, slot: int, page_list, stream=None) -> None:
        """Install or replace slot's page table (rc_index_pages_set; an empty list frees it):
        position p of the slot lives at local row ``page_list[p // 256] * 256 + p % 256``."""
        arr = np.ascontiguousarray(page_list, dtype=np.int32).reshape(-1)
        check(self.lib.rc_index_pages_set(self.handle, int(slot), arr.ctypes.data if arr.size else None, int(arr.size),
                                          stream_ptr(stream)))

    def search_pages(self, queries: torch.Tensor, k: int, slot: int, n_pos: int, stream=None, mask=None, mode: str = "scan"):
        """``search`` over positions [0, n_pos) of a slot (rc_index_search_pages_ex): the rows
        returned are ``row_base + position * row_stride``.  ``mask``: an optional device bitmap
        over the positions, as ``search`` takes one over the rows.  ``mode``: "scan" (default),
        "mfma" / "mfma_masked" (the batched MFMA search over the slot's pages: an f16/bf16 index
        with the native or the "metric" filter, else the library's unsupported error; the scan's
        bits) or "auto" (scans with a mask; without one the batched search where it is available,
        from 64 queries over 65536 positions or 16 queries over 262144)."""
        if mode not in _lib.SEARCH_MODES:
            raise ValueError(f"unknown search mode {mode!r}")
        q = self._vecs(queries)
        nq = q.shape[0]
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        rows = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        if mask is not None:
            if mask.dtype not in (torch.int32, torch.uint32) or mask.numel() < (int(n_pos) + 31) // 32:
                raise ValueError("mask must hold ceil(n_pos / 32) 32-bit words")
            mask = mask.to(device=self.device).contiguous()
        check(self.lib.rc_index_search_pages_ex(self.handle, ptr(q), nq, int(slot), int(n_pos), int(k), ptr(mask), ptr(scores),
                                                ptr(rows), _lib.SEARCH_MODES[mode], stream_ptr(stream)))
        return scores, rows

    def _device_mask(self, mask, n: int):
        if mask is None:
            return None
        if mask.dtype not in (torch.int32, torch.uint32) or mask.numel() < (int(n) + 31) // 32:
            raise ValueError("mask must hold ceil(n / 32) 32-bit words")
        return mask.to(device=self.device).contiguous()

    def search_deep(self, queries: torch.Tensor, k: int, n_rows: int, stream=None, mask=None):
        """Exact top-k for ``k`` up to 10000 (rc_index_search_deep): one pass over the rows that
        keeps every row's score, then ``ceil(k / 256)`` selection rounds over the scores.  The
        scores, rows and tie order of ``search(mode="scan")`` continued past 256; slots past the
        eligible rows are ``(-inf, -1)``.  ``mask``: as ``search`` (a device bitmap over the
        local rows).  Works on every dtype, metric and filter kind."""
        q = self._vecs(queries)
        nq = q.shape[0]
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        rows = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        mask = self._device_mask(mask, n_rows)
        check(self.lib.rc_index_search_deep(self.handle, ptr(q), nq, int(n_rows), int(k), ptr(mask), ptr(scores), ptr(rows),
                                            stream_ptr(stream)))
        return scores, rows

    def search_pages_deep(self, queries: torch.Tensor, k: int, slot: int, n_pos: int, stream=None, mask=None):
        """``search_deep`` over positions [0, n_pos) of a slot (rc_index_search_pages_deep)."""
        q = self._vecs(queries)
        nq = q.shape[0]
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        rows = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        mask = self._device_mask(mask, n_pos)
        check(self.lib.rc_index_search_pages_deep(self.handle, ptr(q), nq, int(slot), int(n_pos), int(k), ptr(mask), ptr(scores),
                                                  ptr(rows), stream_ptr(stream)))
        return scores, rows

    def scores(self, query: torch.Tensor, n_rows: int, slot: int | None = None, stream=None) -> torch.Tensor:
        """A diagnostic (rc_index_scores): the deep search's score pass alone, f32 [n_rows] = the
        score of one raw query against every local row — the bits every search path gives that
        row.  ``slot``: the positions [0, n_rows) of that slot instead (rc_index_scores_pages)."""
        q = self._vecs(query)
        if q.shape[0] != 1:
            raise ValueError("scores takes one query")
        out = torch.empty((int(n_rows),), dtype=torch.float32, device=self.device)
        if slot is None:
            check(self.lib.rc_index_scores(self.handle, ptr(q), int(n_rows), ptr(out), stream_ptr(stream)))
        else:
            check(self.lib.rc_index_scores_pages(self.handle, ptr(q), int(slot), int(n_rows), ptr(out), stream_ptr(stream)))
        return out

    # ------------------------------------------------------------ sparse-dense hybrid --
    def sparse_enable(self, width: int, stream=None) -> None:
        """Give this shard its sparse store (rc_index_sparse_enable): ``width`` slots of (index,
        value) per local row, 8 * width * capacity bytes; it grows with ``grow``."""
        check(self.lib.rc_index_sparse_enable(self.handle, int(width), stream_ptr(stream)))

    @property
    def sparse_width(self) -> int:
        w = _lib.C.c_int()
        check(self.lib.rc_index_sparse_width(self.handle, _lib.C.byref(w)))
        return w.value

    def sparse_write(self, rows, sparse, stream=None) -> None:
        """The sparse values of local rows (rc_index_sparse_write; synchronous): ``sparse[i]`` (a
        ``{"indices", "values"}`` dict, its normal form, or ``None`` for none) replaces every slot
        of row ``rows[i]``."""
        rows = np.ascontiguousarray(torch.as_tensor(rows, dtype=torch.int64).cpu().numpy().reshape(-1))
        if rows.shape[0] != len(sparse):
            raise ValueError("rows and sparse values differ in length")
        off, idx, val = sparsevalues.csr([sparsevalues.normalize(sp, sparsevalues.MAX_NNZ) for sp in sparse])
        check(self.lib.rc_index_sparse_write(self.handle, rows.ctypes.data, off.ctypes.data, idx.ctypes.data, val.ctypes.data,
                                             rows.shape[0], stream_ptr(stream)))

    @staticmethod
    def _sparse_queries(sparse, nq: int):
        """The sparse parts of ``nq`` queries as the host CSR the hybrid calls take."""
        if len(sparse) != nq:
            raise ValueError("queries and sparse vectors differ in length")
        return sparsevalues.csr([sparsevalues.normalize(sp, sparsevalues.MAX_NNZ, "sparse_vector") for sp in sparse], np.int32)

    def search_hybrid(self, queries: torch.Tensor, k: int, n_rows: int, sparse, stream=None, mask=None):
        """``search_deep`` on ``dense . dense + sparse . sparse`` (rc_index_search_hybrid; a
        dotproduct index with a sparse store): ``sparse[q]`` is query q's sparse part (``None`` =
        none).  The score is ``fadd(d, t)``: ``d`` what ``scores`` gives the row, ``t`` the
        row's sparse term (``sparsevalues.model_term``); for any ``k`` up to 10000."""
        q = self._vecs(queries)
        nq = q.shape[0]
        off, idx, val = self._sparse_queries(sparse, nq)
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        rows = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        mask = self._device_mask(mask, n_rows)
        check(self.lib.rc_index_search_hybrid(self.handle, ptr(q), nq, int(n_rows), int(k), ptr(mask), off.ctypes.data,
                                              idx.ctypes.data, val.ctypes.data, ptr(scores), ptr(rows), stream_ptr(stream)))
        return scores, rows

    def search_pages_hybrid(self, queries: torch.Tensor, k: int, slot: int, n_pos: int, sparse, stream=None, mask=None):
        """``search_hybrid`` over positions [0, n_pos) of a slot (rc_index_search_pages_hybrid)."""
        q = self._vecs(queries)
        nq = q.shape[0]
        off, idx, val = self._sparse_queries(sparse, nq)
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        rows = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        mask = self._device_mask(mask, n_pos)
        check(self.lib.rc_index_search_pages_hybrid(self.handle, ptr(q), nq, int(slot), int(n_pos), int(k), ptr(mask),
                                                    off.ctypes.data, idx.ctypes.data, val.ctypes.data, ptr(scores), ptr(rows),
                                                    stream_ptr(stream)))
        return scores, rows

    def scores_hybrid(self, query: torch.Tensor, n_rows: int, sparse, slot: int | None = None, stream=None) -> torch.Tensor:
        """A diagnostic (rc_index_scores_hybrid): ``scores`` plus the sparse add kernel for one
        query — the hybrid score of every local row (``slot``: position) before any selection."""
        q = self._vecs(query)
        if q.shape[0] != 1:
            raise ValueError("scores_hybrid takes one query")
        off, idx, val = self._sparse_queries([sparse], 1)
        out = torch.empty((int(n_rows),), dtype=torch.float32, device=self.device)
        check(self.lib.rc_index_scores_hybrid(self.handle, ptr(q), -1 if slot is None else int(slot), int(n_rows), off.ctypes.data,
                                              idx.ctypes.data, val.ctypes.data, ptr(out), stream_ptr(stream)))
        return out

    def export_rows(self, row0: int, n: int, stream=None):
        """Raw stored rows [row0, row0+n) (storage dtype bits, ld-padded) and norms, on the device."""
        el = _lib.dtype_bytes(self.dtype)
        rows = torch.empty((n, self.ld * el), dtype=torch.uint8, device=self.device)
        norms = torch.empty((n,), dtype=torch.float32, device=self.device)
        check(self.lib.rc_index_export(self.handle, int(row0), int(n), ptr(rows), ptr(norms), stream_ptr(stream)))
        return rows, norms

    def import_rows(self, row0: int, rows: torch.Tensor, norms: torch.Tensor, stream=None) -> None:
        """Inverse of export_rows: write raw stored rows + norms at [row0, row0+n)."""
        el = _lib.dtype_bytes(self.dtype)
        rows = rows.to(device=self.device, dtype=torch.uint8).contiguous()
        norms = norms.to(device=self.device, dtype=torch.float32).contiguous()
        n = norms.numel()
        if rows.numel() != n * self.ld * el:
            raise ValueError("row bytes do not match the index layout (dimension / dtype)")
        check(self.lib.rc_index_import(self.handle, int(row0), n, ptr(rows), ptr(norms), stream_ptr(stream)))

    def fill_random(self, seed: int, row0: int, n: int, stream=None) -> None:
        check(self.lib.rc_index_fill_random(self.handle, int(seed), int(row0), int(n), stream_ptr(stream)))

    def stored_rows(self, rows: "torch.Tensor | int", stream=None) -> torch.Tensor:
        """The stored (normalised, dtype-rounded) rows as f32 — what search scores against."""
        if isinstance(rows, int):
            rows = torch.arange(rows, dtype=torch.int64)
        rows = rows.to(device=self.device, dtype=torch.int64).contiguous()
        out = torch.empty((rows.numel(), self.dim), dtype=torch.float32, device=self.device)
        check(self.lib.rc_index_fetch_stored(self.handle, ptr(rows), rows.numel(), ptr(out), stream_ptr(stream)))
        return out

    def timing(self, enable: bool) -> None:
        check(self.lib.rc_index_timing(self.handle, 1 if enable else 0))

    def timing_read(self):
        """Scan kernel: (total ms, launches, algorithmic bytes) since the last read."""
        ms = _lib.C.c_double()
        n = _lib.C.c_int64()
        b = _lib.C.c_double()
        check(self.lib.rc_index_timing_read(self.handle, _lib.C.byref(ms), _lib.C.byref(n), _lib.C.byref(b)))
        return ms.value, n.value, b.value

    def gemm_timing_read(self):
        """Batched filter GEMM: (total ms, launches, flops, fallback count) since the last read."""
        ms = _lib.C.c_double()
        n = _lib.C.c_int64()
        f = _lib.C.c_double()
        fb = _lib.C.c_int64()
        check(self.lib.rc_index_gemm_timing_read(self.handle, _lib.C.byref(ms), _lib.C.byref(n), _lib.C.byref(f),
                                                 _lib.C.byref(fb)))
        return ms.value, n.value, f.value, fb.value


def topk_merge(scores: torch.Tensor, rows: torch.Tensor, k: int, stream=None):
    """Merge [nlists, nq, k_in] sorted candidate lists into [nq, k] on the device (rc_topk_merge)."""
    lib = _lib.load()
    scores = scores.contiguous()
    rows = rows.contiguous()
    nlists, nq, k_in = scores.shape
    out_s = torch.empty((nq, k), dtype=torch.float32, device=scores.device)
    out_r = torch.empty((nq, k), dtype=torch.int64, device=scores.device)
    check(lib.rc_topk_merge(ptr(scores), ptr(rows), nlists, nq, k_in, k, ptr(out_s), ptr(out_r), stream_ptr(stream)))
    return out_s, out_r


class Record(dict):
    """A query match or fetched vector in Pinecone's shape (``{"id", "score" | "values",
    "metadata"}``) whose ``"values"`` entry stays a float32 row until something reads it.

    The reference's ``search`` asks for ``include_values=True`` and keeps only the ids
    (``retriever/utils.py:62-65``), so building 5 x 768 Python floats per request is work no
    caller of that path sees.  Every read path of the dict — ``[]``, ``get``, ``items``,
    ``values``, iteration with ``dict(...)`` / ``{**m}``, ``==``, ``copy``, ``repr``, pickling,
    ``json.dumps`` (which calls ``items()`` on a dict subclass), ``|`` — first turns the row into
    the list of Python floats a plain dict would hold, once; writing or deleting ``"values"``
    drops the pending row, and ``update`` / ``|=`` load it first."""

    __slots__ = ("_row",)

    def __init__(self, row: np.ndarray | None = None, **fields):
        super().__init__(fields)
        self._row = row
        if row is not None:
            dict.__setitem__(self, "values", None)

    def _load(self) -> None:
        row = self._row
        if row is not None:
            self._row = None
            dict.__setitem__(self, "values", row.astype(np.float64).tolist())

    def __getitem__(self, key):
        if key == "values":
            self._load()
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        if key == "values":
            self._load()
        return dict.get(self, key, default)

    def __iter__(self):  # a Python-level __iter__ sends dict(m) / {**m} through keys() + __getitem__
        return dict.__iter__(self)

    def items(self):
        self._load()
        return dict.items(self)

    def values(self):
        self._load()
        return dict.values(self)

    def copy(self):
        self._load()
        return dict(dict.items(self))

    def pop(self, key, *default):
        self._load()
        return dict.pop(self, key, *default)

    def popitem(self):
        self._load()
        return dict.popitem(self)

    def setdefault(self, key, default=None):
        self._load()
        return dict.setdefault(self, key, default)

    # writes: a new "values" (or its removal) supersedes the pending row, so the row must not
    # come back on the next read; any other key leaves it pending
    def __setitem__(self, key, value):
        if key == "values":
            self._row = None
        dict.__setitem__(self, key, value)

    def __delitem__(self, key):
        if key == "values":
            self._row = None
        dict.__delitem__(self, key)

    def update(self, *a, **kw):
        self._load()
        dict.update(self, *a, **kw)

    def __or__(self, other):
        self._load()
        return dict(dict.items(self)) | dict(other)

    def __ror__(self, other):
        self._load()
        return dict(other) | dict(dict.items(self))

    def __ior__(self, other):
        self.update(other)
        return self

    def __eq__(self, other):
        self._load()
        if isinstance(other, Record):
            other._load()
        return dict.__eq__(self, other)

    def __ne__(self, other):
        return not self.__eq__(other)

    __hash__ = None

    def __repr__(self):
        self._load()
        return dict.__repr__(self)

    def __reduce__(self):
        self._load()
        return (dict, (dict(dict.items(self)),))


class F32List(list):
    """A list of floats (an embedding as ``/embed`` returns it) that also carries the float32
    array it was made from, so an in-process ``search`` (retriever/main.py:122-128: the
    feature goes straight back into ``index.query``) skips re-parsing 768 Python floats.  Any
    mutation drops the array; the list is then parsed like any other."""

    __slots__ = ("f32",)

    def __init__(self, values=(), f32: np.ndarray | None = None):
        super().__init__(values)
        self.f32 = f32

    def __setitem__(self, *a):
        self.f32 = None
        return list.__setitem__(self, *a)

    def __delitem__(self, *a):
        self.f32 = None
        return list.__delitem__(self, *a)

    def __iadd__(self, other):
        self.f32 = None
        return list.__iadd__(self, other)

    def __imul__(self, n):
        self.f32 = None
        return list.__imul__(self, n)

    def __reduce__(self):  # pickles / copies as the plain list
        return (list, (list(self),))


def _invalidating(name):
    base = getattr(list, name)

    def method(self, *a, **k):
        self.f32 = None
        return base(self, *a, **k)

    method.__name__ = name
    return method


for _m in ("append", "extend", "insert", "pop", "remove", "reverse", "sort", "clear"):
    setattr(F32List, _m, _invalidating(_m))
del _m


def _as_vector(values: Any, dim: int) -> list[float]:
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().reshape(-1).tolist()
    vals = [float(v) for v in values]
    if len(vals) != dim:
        raise ValueError(f"Vector dimension {len(vals)} does not match the dimension of the index {dim}")
    if not any(v != 0.0 for v in vals):
        raise ValueError("Dense vectors must contain at least one non-zero value for the cosine metric")
    return vals


def _as_vector_np(values: Any, dim: int) -> np.ndarray:
    """``_as_vector`` as a C-contiguous f32 [1, dim] host array (the request path: no per-element
    Python loop)."""
    if type(values) is F32List and values.f32 is not None:  # an in-process embedding: its own f32 row
        a = values.f32
    elif isinstance(values, torch.Tensor):
        a = values.detach().to(device="cpu", dtype=torch.float32).reshape(-1).numpy()
    else:
        a = None
        if isinstance(values, (list, tuple)):
            try:  # a JSON list of floats: array('f') converts it ~4x faster than np.asarray (same f32 rounding)
                a = np.frombuffer(array.array("f", values), dtype=np.float32)
            except TypeError:
                pass
        if a is None:
            a = np.asarray(values, dtype=np.float32)
            if a.ndim != 1:  # as _as_vector: float() of a nested element raises, nothing is flattened
                raise TypeError(f"a query vector must be a flat sequence of numbers (got shape {a.shape})")
    if a.shape[0] != dim:
        raise ValueError(f"Vector dimension {a.shape[0]} does not match the dimension of the index {dim}")
    if not a.any():
        raise ValueError("Dense vectors must contain at least one non-zero value for the cosine metric")
    return np.ascontiguousarray(a[None])


class ShardSet:
    """One ``rc_sharded`` handle: ``n`` shards (``rc_index`` each) in this process.

    Global row g lives on shard ``g % n`` as local row ``g // n`` (round-robin,
    SURVEY §8(e)); ``devices[s]`` is shard s's GPU (entries may repeat), and
    ``devices[0]`` (the leader) holds queries and merged results."""

    def __init__(self, dim: int, dtype: str = "float32", capacity_per_shard: int = 1 << 20, devices=None,
                 metric: str = "cosine"):
        self.lib = _lib.load()
        if dtype not in _lib.DTYPES:
            raise ValueError(f"unknown index dtype {dtype!r}")
        if metric not in _lib.METRICS:
            raise ValueError(f"unknown metric {metric!r} (expected one of {sorted(_lib.METRICS)})")
        devs = [_device_index(d) for d in (devices if devices is not None else [None])]
        if not devs:
            raise ValueError("a sharded index needs at least one device")
        self.dim = int(dim)
        self.dtype = dtype
        self.devices = devs
        self.n = len(devs)
        self.device = torch.device("cuda", devs[0])
        arr = (_lib.C.c_int * self.n)(*devs)
        h = _lib.C.c_void_p()
        check(self.lib.rc_sharded_create(self.n, arr, self.dim, _lib.DTYPES[dtype], int(capacity_per_shard),
                                         _lib.C.byref(h)))
        self._h = h
        # rows upsert_parts had to copy from another GPU than their shard's (an EmbedderPool
        # batch whose planned rows shifted under a concurrent ingest): results stay exact,
        # this counts the extra xGMI traffic
        self.cross_device_rows = 0
        self._qbufs: dict = {}  # query_host's reused host buffers per (nq, k, values)
        self._query_fn = self.lib.rc_sharded_query_host
        self._query_masked_fn = self.lib.rc_sharded_query_host_masked
        self._shards = []
        for sh in range(self.n):
            ih = _lib.C.c_void_p()
            check(self.lib.rc_sharded_shard(h, sh, _lib.C.byref(ih)))
            self._shards.append(DeviceIndex(dim, dtype=dtype, device=devs[sh], row_base=sh, row_stride=self.n, _handle=ih))
        if metric != "cosine":
            self.set_metric(metric)

    @property
    def handle(self):
        if self._h is None:
            raise RuntimeError("index is closed")
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            for d in self._shards:
                d.close()
            check(self.lib.rc_sharded_destroy(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def capacity_per_shard(self) -> int:
        cap = _lib.C.c_int64()
        check(self.lib.rc_sharded_info(self.handle, None, _lib.C.byref(cap), None))
        return cap.value

    @property
    def capacity(self) -> int:
        return self.capacity_per_shard * self.n

    @property
    def ld(self) -> int:
        ld = _lib.C.c_int64()
        check(self.lib.rc_sharded_info(self.handle, None, None, _lib.C.byref(ld)))
        return ld.value

    def force_remote(self) -> None:
        """Test hook (rc_sharded_force_remote): every shard but the leader through the
        cross-device path, as on a multi-GPU node, even when the shards share one GPU."""
        check(self.lib.rc_sharded_force_remote(self.handle))

    def shard(self, s: int) -> DeviceIndex:
        return self._shards[s]

    def shard_rows(self, s: int, n_rows: int) -> int:
        """How many of the global rows [0, n_rows) shard s holds."""
        return (n_rows - s + self.n - 1) // self.n if n_rows > s else 0

    def grow(self, new_capacity_per_shard: int) -> None:
        check(self.lib.rc_sharded_grow(self.handle, int(new_capacity_per_shard)))

    def set_filter(self, kind: str) -> None:
        """``DeviceIndex.set_filter`` on every shard."""
        if kind not in _lib.FILTERS:
            raise ValueError(f"unknown filter {kind!r} (expected one of {sorted(_lib.FILTERS)})")
        check(self.lib.rc_sharded_set_filter(self.handle, _lib.FILTERS[kind]))

    @property
    def filter(self) -> str:
        return self._shards[0].filter

    def set_metric(self, metric: str) -> None:
        """``DeviceIndex.set_metric`` on every shard (rc_sharded_set_metric: all or none)."""
        if metric not in _lib.METRICS:
            raise ValueError(f"unknown metric {metric!r} (expected one of {sorted(_lib.METRICS)})")
        check(self.lib.rc_sharded_set_metric(self.handle, _lib.METRICS[metric]))

    @property
    def metric(self) -> str:
        return self._shards[0].metric

    def upsert_rows(self, vecs: torch.Tensor, rows) -> None:
        """vecs f32 [n, dim] (any device; moved to the leader), rows: global rows (host)."""
        if vecs.dim() == 1:
            vecs = vecs[None]
        if vecs.shape[-1] != self.dim:
            raise ValueError(f"Vector dimension {vecs.shape[-1]} does not match the dimension of the index {self.dim}")
        vecs = vecs.to(device=self.device, dtype=torch.float32).contiguous()
        rows = torch.as_tensor(rows, dtype=torch.int64).cpu().contiguous()
        if rows.numel() != vecs.shape[0]:
            raise ValueError("rows and vectors differ in length")
        check(self.lib.rc_sharded_upsert(self.handle, ptr(vecs), vecs.shape[0], ptr(rows), stream_ptr(None)))

    def move_rows(self, src, dst) -> None:
        """Stored global row dst[i] becomes a copy of stored global row src[i]
        (rc_sharded_move_rows; host lists, validated there: in capacity, no row twice in either
        list, none in both).  Synchronous."""
        src = torch.as_tensor(src, dtype=torch.int64).cpu().contiguous()
        dst = torch.as_tensor(dst, dtype=torch.int64).cpu().contiguous()
        if src.numel() != dst.numel():
            raise ValueError("src and dst differ in length")
        check(self.lib.rc_sharded_move_rows(self.handle, ptr(src), ptr(dst), src.numel()))

    def upsert_parts(self, parts) -> None:
        """Upsert vectors that already live on several devices (an ``EmbedderPool`` batch):
        ``parts`` = [(global rows: host i64 [m], vecs: f32 [m, dim] on any GPU)].  Each part's
        rows go straight to their shards: a shard on the part's own device takes its subset
        in place (no copy at all when the pool member and the shard share the GPU, the
        common case), any other shard gets only its subset copied over.  Synchronous per
        shard device, like ``upsert_rows``."""
        touched = set()
        for rows, vecs in parts:
            rows = torch.as_tensor(rows, dtype=torch.int64).cpu().reshape(-1)
            if rows.numel() == 0:
                continue
            if vecs.dim() != 2 or vecs.shape[0] != rows.numel() or vecs.shape[1] != self.dim:
                raise ValueError("each part needs vecs [len(rows), dim]")
            if int(rows.min()) < 0 or int(rows.max()) // self.n >= self.capacity_per_shard:
                raise ValueError("row out of capacity")
            sh = torch.remainder(rows, self.n)
            for s in torch.unique(sh).tolist():
                sel = torch.nonzero(sh == s).reshape(-1)
                d = self.devices[s]
                if vecs.device != torch.device("cuda", d):
                    self.cross_device_rows += int(sel.numel())
                v = vecs if sel.numel() == rows.numel() else vecs[sel.to(vecs.device)]
                with torch.cuda.device(d):
                    v = v.to(device=torch.device("cuda", d), dtype=torch.float32).contiguous()
                    self._shards[s].upsert_rows(v, torch.div(rows[sel], self.n, rounding_mode="floor"))
                touched.add(d)
        for d in touched:
            torch.cuda.synchronize(d)

    @staticmethod
    def _host_mask(mask, n_rows: int) -> np.ndarray:
        """A host bitmap over the global rows as C-contiguous uint32 [>= ceil(n_rows / 32)]."""
        m = np.ascontiguousarray(mask, dtype=np.uint32).reshape(-1)
        if m.shape[0] < (int(n_rows) + 31) // 32:
            raise ValueError("mask must hold ceil(n_rows / 32) uint32 words")
        return m

    def query_host(self, q: np.ndarray, k: int, n_rows: int, with_values: bool, mask=None):
        """Host f32 [nq, dim] → host (scores [nq, k], global rows [nq, k], values [nq, k, dim] or
        None): rc_sharded_query_host — one H2D copy, the search and the matched rows' gather, one
        D2H copy, one synchronisation.  The arrays are this ShardSet's reused buffers: valid
        until its next query_host call (the Index consumes them under its lock).  ``mask``: an
        optional HOST uint32 bitmap over the global rows (rc_sharded_query_host_masked)."""
        nq = int(q.shape[0])
        key = (nq, int(k), bool(with_values))
        bufs = self._qbufs.get(key)
        if bufs is None:
            if len(self._qbufs) > 16:
                self._qbufs.clear()
            sc = np.empty((nq, k), np.float32)
            rw = np.empty((nq, k), np.int64)
            val = np.empty((nq, k, self.dim), np.float32) if with_values else None
            # the buffers' addresses once (ctypes attribute reads cost ~1 us each per call)
            ptrs = (int(bool(with_values)), sc.ctypes.data, rw.ctypes.data, val.ctypes.data if val is not None else None)
            bufs = (sc, rw, val, ptrs)
            self._qbufs[key] = bufs
        sc, rw, val, ptrs = bufs
        h = self._h
        if h is None:
            raise RuntimeError("index is closed")
        if mask is None:
            check(self._query_fn(h, q.ctypes.data, nq, n_rows, k, ptrs[0], ptrs[1], ptrs[2], ptrs[3]))
        else:
            m = self._host_mask(mask, n_rows)
            check(self._query_masked_fn(h, q.ctypes.data, nq, n_rows, k, ptrs[0], m.ctypes.data, ptrs[1], ptrs[2], ptrs[3]))
        return sc, rw, val

    def fetch_rows(self, rows, stored: bool = False) -> torch.Tensor:
        """Host f32 [n, dim]: the upserted values (or, ``stored``, the normalised stored rows)."""
        rows = torch.as_tensor(rows, dtype=torch.int64).cpu().contiguous()
        out = torch.empty((rows.numel(), self.dim), dtype=torch.float32)
        if rows.numel():
            check(self.lib.rc_sharded_fetch(self.handle, ptr(rows), rows.numel(), ptr(out), 1 if stored else 0))
        return out

    def search(self, queries: torch.Tensor, k: int, n_rows: int, mode: str = "auto", stream=None, mask=None):
        """Exact top-k over global rows [0, n_rows) by the index's metric: (scores f32 [nq,k]
        descending, rows i64 [nq,k]) on the leader.
        ``mask``: an optional HOST uint32 bitmap over the global rows (rc_sharded_search_masked);
        ``mode="mfma_masked"`` runs every shard's filter GEMM under its part of the mask
        (``DeviceIndex.search``)."""
        if mode not in _lib.SEARCH_MODES:
            raise ValueError(f"unknown search mode {mode!r}")
        if queries.dim() == 1:
            queries = queries[None]
        q = queries.to(device=self.device, dtype=torch.float32).contiguous()
        nq = q.shape[0]
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        rows = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        if mask is None:
            check(self.lib.rc_sharded_search(self.handle, ptr(q), nq, int(n_rows), int(k), ptr(scores), ptr(rows),
                                             _lib.SEARCH_MODES[mode], stream_ptr(stream)))
        else:
            m = self._host_mask(mask, n_rows)
            check(self.lib.rc_sharded_search_masked(self.handle, ptr(q), nq, int(n_rows), int(k), m.ctypes.data,
                                                    ptr(scores), ptr(rows), _lib.SEARCH_MODES[mode], stream_ptr(stream)))
        return scores, rows

    # ------------------------------------------------------------------ page tables --
    # A slot is one vector set (a namespace) inside this ShardSet's rows: an ordered list of
    # pages (``pages``: RC_PAGE_ROWS local rows on every shard each) holding positions [0, n_pos).
    # Rows are written, fetched and moved by global row as ever; only the searches go through
    # the table, and they return POSITIONS (retrieval_core.h, "Page tables").
    def set_pages(self, slot: int, page_list) -> None:
        """Install or replace slot's page table on every shard (rc_sharded_pages_set); an empty
        list frees it.  Waits for the devices: call it when the set gains or loses a page."""
        arr = np.ascontiguousarray(page_list, dtype=np.int32).reshape(-1)
        check(self.lib.rc_sharded_pages_set(self.handle, int(slot), arr.ctypes.data if arr.size else None, int(arr.size)))

    def search_pages(self, queries: torch.Tensor, k: int, slot: int, n_pos: int, stream=None, mask=None, mode: str = "scan"):
        """``search`` over the positions [0, n_pos) of a slot: (scores, positions), bit-identical
        to a dense ShardSet of as many shards holding the slot's vectors in position order.
        ``mask``: an optional HOST uint32 bitmap over the positions.  ``mode``: as
        ``DeviceIndex.search_pages``; every shard takes it (rc_sharded_search_pages_ex)."""
        if mode not in _lib.SEARCH_MODES:
            raise ValueError(f"unknown search mode {mode!r}")
        if queries.dim() == 1:
            queries = queries[None]
        q = queries.to(device=self.device, dtype=torch.float32).contiguous()
        nq = q.shape[0]
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        rows = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        m = None if mask is None else self._host_mask(mask, n_pos)
        check(self.lib.rc_sharded_search_pages_ex(self.handle, ptr(q), nq, int(slot), int(n_pos), int(k),
                                                  None if m is None else m.ctypes.data, ptr(scores), ptr(rows),
                                                  _lib.SEARCH_MODES[mode], stream_ptr(stream)))
        return scores, rows

    def search_deep(self, queries: torch.Tensor, k: int, n_rows: int, stream=None, mask=None):
        """``search`` for ``k`` up to 10000 (rc_sharded_search_deep; ``DeviceIndex.search_deep``):
        every shard selects its own ``k``, the leader selects among the shards' lists — the
        result of a single-shard index holding the same rows.  ``mask``: an optional HOST uint32
        bitmap over the global rows."""
        if queries.dim() == 1:
            queries = queries[None]
        q = queries.to(device=self.device, dtype=torch.float32).contiguous()
        nq = q.shape[0]
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        rows = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        m = None if mask is None else self._host_mask(mask, n_rows)
        check(self.lib.rc_sharded_search_deep(self.handle, ptr(q), nq, int(n_rows), int(k), None if m is None else m.ctypes.data,
                                              ptr(scores), ptr(rows), stream_ptr(stream)))
        return scores, rows

    def search_pages_deep(self, queries: torch.Tensor, k: int, slot: int, n_pos: int, stream=None, mask=None):
        """``search_deep`` over the positions [0, n_pos) of a slot (rc_sharded_search_pages_deep):
        (scores, positions).  ``mask``: an optional HOST uint32 bitmap over the positions."""
        if queries.dim() == 1:
            queries = queries[None]
        q = queries.to(device=self.device, dtype=torch.float32).contiguous()
        nq = q.shape[0]
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        rows = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        m = None if mask is None else self._host_mask(mask, n_pos)
        check(self.lib.rc_sharded_search_pages_deep(self.handle, ptr(q), nq, int(slot), int(n_pos), int(k),
                                                    None if m is None else m.ctypes.data, ptr(scores), ptr(rows),
                                                    stream_ptr(stream)))
        return scores, rows

    # ------------------------------------------------------------ sparse-dense hybrid --
    def sparse_enable(self, width: int) -> None:
        """``DeviceIndex.sparse_enable`` on every shard (rc_sharded_sparse_enable)."""
        check(self.lib.rc_sharded_sparse_enable(self.handle, int(width)))

    @property
    def sparse_width(self) -> int:
        return self._shards[0].sparse_width

    def sparse_write(self, rows, sparse) -> None:
        """``DeviceIndex.sparse_write`` by GLOBAL row (rc_sharded_sparse_write; host lists,
        synchronous): row g is local row g // n of shard g % n."""
        rows = np.ascontiguousarray(torch.as_tensor(rows, dtype=torch.int64).cpu().numpy().reshape(-1))
        if rows.shape[0] != len(sparse):
            raise ValueError("rows and sparse values differ in length")
        if rows.shape[0] == 0:
            return
        off, idx, val = sparsevalues.csr([sparsevalues.normalize(sp, sparsevalues.MAX_NNZ) for sp in sparse])
        check(self.lib.rc_sharded_sparse_write(self.handle, rows.ctypes.data, off.ctypes.data, idx.ctypes.data, val.ctypes.data,
                                               rows.shape[0]))

    def search_hybrid(self, queries: torch.Tensor, k: int, n_rows: int, sparse, stream=None, mask=None):
        """``search_deep`` on ``dense . dense + sparse . sparse`` (rc_sharded_search_hybrid;
        ``DeviceIndex.search_hybrid``): every shard adds its rows' sparse terms to its own scores
        before it selects — the result of a single-shard index holding the same records.
        ``mask``: an optional HOST uint32 bitmap over the global rows."""
        if queries.dim() == 1:
            queries = queries[None]
        q = queries.to(device=self.device, dtype=torch.float32).contiguous()
        nq = q.shape[0]
        off, idx, val = DeviceIndex._sparse_queries(sparse, nq)
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        rows = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        m = None if mask is None else self._host_mask(mask, n_rows)
        check(self.lib.rc_sharded_search_hybrid(self.handle, ptr(q), nq, int(n_rows), int(k), None if m is None else m.ctypes.data,
                                                off.ctypes.data, idx.ctypes.data, val.ctypes.data, ptr(scores), ptr(rows),
                                                stream_ptr(stream)))
        return scores, rows

    def search_pages_hybrid(self, queries: torch.Tensor, k: int, slot: int, n_pos: int, sparse, stream=None, mask=None):
        """``search_hybrid`` over the positions [0, n_pos) of a slot (rc_sharded_search_pages_hybrid):
        (scores, positions).  ``mask``: an optional HOST uint32 bitmap over the positions."""
        if queries.dim() == 1:
            queries = queries[None]
        q = queries.to(device=self.device, dtype=torch.float32).contiguous()
        nq = q.shape[0]
        off, idx, val = DeviceIndex._sparse_queries(sparse, nq)
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        rows = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        m = None if mask is None else self._host_mask(mask, n_pos)
        check(self.lib.rc_sharded_search_pages_hybrid(self.handle, ptr(q), nq, int(slot), int(n_pos), int(k),
                                                      None if m is None else m.ctypes.data, off.ctypes.data, idx.ctypes.data,
                                                      val.ctypes.data, ptr(scores), ptr(rows), stream_ptr(stream)))
        return scores, rows

    def scores_hybrid(self, query: torch.Tensor, n_rows: int, sparse, slot: int | None = None) -> torch.Tensor:
        """``DeviceIndex.scores_hybrid`` of every shard, interleaved into global row (``slot``:
        position) order on the leader: f32 [n_rows].  A diagnostic; it waits for each shard."""
        out = torch.empty((int(n_rows),), dtype=torch.float32, device=self.device)
        for s, sh in enumerate(self._shards):
            m = self.shard_rows(s, int(n_rows))
            if m == 0:
                continue
            with torch.cuda.device(sh.device):
                part = sh.scores_hybrid(query.to(sh.device), m, sparse, slot=slot)
                torch.cuda.synchronize(sh.device)
            out[s::self.n] = part.to(self.device)
        return out

    def query_host_pages(self, q: np.ndarray, k: int, slot: int, n_pos: int, with_values: bool, mask=None):
        """``query_host`` over the positions [0, n_pos) of a slot (rc_sharded_query_host_pages):
        host (scores, positions, values or None), new arrays."""
        nq = int(q.shape[0])
        sc = np.empty((nq, k), np.float32)
        rw = np.empty((nq, k), np.int64)
        val = np.empty((nq, k, self.dim), np.float32) if with_values else None
        m = None if mask is None else self._host_mask(mask, n_pos)
        check(self.lib.rc_sharded_query_host_pages(self.handle, q.ctypes.data, nq, int(slot), int(n_pos), int(k),
                                                   1 if with_values else 0, None if m is None else m.ctypes.data,
                                                   sc.ctypes.data, rw.ctypes.data, None if val is None else val.ctypes.data))
        return sc, rw, val

    def export_run(self, row0: int, n: int):
        """Raw stored rows and norms of the global rows [row0, row0 + n), ``row0`` a multiple of
        the shard count (a run of pages): each shard's part is one contiguous block."""
        if row0 % self.n:
            raise ValueError("row0 must be a multiple of the shard count")
        el = _lib.dtype_bytes(self.dtype)
        rows = np.zeros((n, self.ld * el), dtype=np.uint8)
        norms = np.zeros((n,), dtype=np.float32)
        for s in range(self.n):
            m = self.shard_rows(s, n)
            if m == 0:
                continue
            r, nr = self._shards[s].export_rows(row0 // self.n, m)
            torch.cuda.synchronize(self._shards[s].device)
            rows[s::self.n] = r.cpu().numpy()
            norms[s::self.n] = nr.cpu().numpy()
        return rows, norms

    def import_run(self, row0: int, rows, norms) -> None:
        """Inverse of ``export_run``."""
        if row0 % self.n:
            raise ValueError("row0 must be a multiple of the shard count")
        for s in range(self.n):
            if self.shard_rows(s, len(norms)) == 0:
                continue
            self._shards[s].import_rows(row0 // self.n, torch.from_numpy(np.ascontiguousarray(rows[s::self.n])),
                                        torch.from_numpy(np.ascontiguousarray(norms[s::self.n])))
            torch.cuda.synchronize(self._shards[s].device)

    # raw stored rows in GLOBAL row order (the snapshot layout, independent of the shard count)
    def export_rows(self, n_rows: int):
        import numpy as np

        el = _lib.dtype_bytes(self.dtype)
        rows = np.zeros((n_rows, self.ld * el), dtype=np.uint8)
        norms = np.zeros((n_rows,), dtype=np.float32)
        for s in range(self.n):
            m = self.shard_rows(s, n_rows)
            if m == 0:
                continue
            r, nr = self._shards[s].export_rows(0, m)
            torch.cuda.synchronize(self._shards[s].device)
            rows[s::self.n] = r.cpu().numpy()
            norms[s::self.n] = nr.cpu().numpy()
        return rows, norms

    def import_rows(self, rows, norms) -> None:
        n_rows = len(norms)
        for s in range(self.n):
            if self.shard_rows(s, n_rows) == 0:
                continue
            self._shards[s].import_rows(0, torch.from_numpy(rows[s::self.n].copy()),
                                        torch.from_numpy(norms[s::self.n].copy()))
            torch.cuda.synchronize(self._shards[s].device)


def _namespace_name(namespace) -> str:
    """``None`` is the default namespace ``""``; anything but a string is refused."""
    if namespace is None:
        return ""
    if not isinstance(namespace, str):
        raise ValueError("namespace must be a string")
    return namespace


# the pool of the named namespaces starts at this many pages per shard and doubles on demand
POOL_INITIAL_PAGES = 4


class _Namespace:
    """Host state of one named namespace: what ``Index`` itself keeps for ``""`` (under the same
    attribute names, so the helpers that take a state serve both), plus its place in the pool —
    the ordered page list and the slot of its device-resident page table.  An id's position is
    its index in ``_ids``; ``pages.position_to_row`` gives the pool row."""

    __slots__ = ("name", "slot", "pages", "_ids", "_rows", "_meta", "_gen", "_recent", "_bitmaps", "_sparse")

    def __init__(self, name: str, slot: int):
        self.name = name
        self.slot = slot
        self.pages: list[int] = []
        self._ids: list[str] = []
        self._rows: dict[str, int] = {}  # id -> position
        self._meta: dict[str, dict] = {}
        self._gen = 0
        self._recent: tuple[int, dict[str, np.ndarray]] = (-1, {})
        self._bitmaps: dict[tuple[str, int], tuple[np.ndarray, int]] = {}
        self._sparse: dict[str, tuple[np.ndarray, np.ndarray]] = {}  # id -> sparse values (sparsevalues' normal form)


class Index:
    """Pinecone-shaped index (what ``get_index`` returns).

    ``metric`` is Pinecone's ``create_index(metric=...)``: ``"cosine"`` (default),
    ``"dotproduct"`` or ``"euclidean"``.  With ``v`` the vector ``fetch`` returns for an id (the
    stored direction, dtype-rounded, times its f32 norm) and ``q`` the raw query, a match's
    score is the cosine, ``q · v`` (higher is better) or the SQUARED distance ``‖q − v‖²`` as
    Pinecone reports it (lower is better).  Matches come most similar first, so Euclidean scores
    ascend; ties order by ascending row under every metric.  The top-k is chosen by the
    metric's score inside the exact scan (the library returns Euclidean scores negated, so
    every search sorts descending; ``query`` / ``query_batch`` report ``max(0.0, -s)``).  The
    metric is a scoring rule over unchanged storage: ``upsert``, ``fetch``, ``delete``,
    ``query(id=...)`` and metadata filters work alike under all three, and ``save`` / ``load``
    keep it.  By default the batched MFMA search is cosine-only: a non-cosine index scans,
    ``mode="mfma"`` and ``filter="i8"`` raise ``ValueError`` on it.  ``filter="metric"`` (an
    f16/bf16 index) gives it the batched search — ``mode="mfma"``, and ``"auto"`` under the
    usual conditions — with the scan's ids and score bits.  All-zero vectors and queries are
    rejected under every metric.

    ``dtype`` is the storage of the normalised rows: ``"float32"``, ``"float16"``, ``"bfloat16"``
    or ``"float8_e4m3fn"`` (alias ``"f8"``: one byte per element, each element of the direction
    rounded to 3 mantissa bits).  A float8 index scans by default (``mode="mfma"`` raises
    ``ValueError``, ``"auto"`` scans); ``filter="f8"`` gives it the batched search on the
    block-scaled fp8 MFMA (cosine, dimensions up to 768), with unchanged results.
    ``filter="i8"`` raises on it, ``filter="f8"`` on every other dtype.

    ``upsert(vectors)`` accepts ``(id, values)``, ``(id, values, metadata)``
    tuples or ``{"id", "values", "metadata"}`` dicts and overwrites existing
    ids (within one call the last occurrence of an id wins); ``query`` returns
    ``{"matches": [{"id", "score", ["values"], ["metadata"]}], "namespace": ""}``
    best first; ``fetch`` returns ``{"vectors": {id: {"id", "values",
    "metadata"}}, "namespace": ""}``; ``delete(ids=... | filter=... | delete_all=True)``
    removes vectors and returns ``{}``.

    The rows live on ``shards`` shards (``devices``: one GPU per shard, entries
    may repeat; default one shard on ``device``), routed round-robin by the
    row number the host assigns each new id, and searched as ONE exact index
    (``rc_sharded``): results are identical to a single-shard index holding the
    same vectors.  Capacity grows on demand (doubling), as a Pinecone index
    has no fixed size.

    Two things are called "filter" here.  The constructor's ``filter="native" | "i8" | "f8" | "metric"`` is
    the kind of filter GEMM the batched search runs (``DeviceIndex.set_filter``); it never
    changes a result.  ``query(..., filter={...})`` / ``query_batch(..., filter={...})`` is
    Pinecone's metadata filter (``metafilter``): only vectors whose metadata satisfies it can
    be returned, and the restriction happens inside the exact search (a row-eligibility
    bitmap the masked scan takes), so the top-k of the eligible vectors is exact however
    selective the filter is.

    ``namespace=`` on ``upsert`` / ``upsert_tensor`` / ``query`` / ``query_batch`` / ``fetch`` /
    ``delete`` names an independent vector set, as in Pinecone: ids are unique per namespace,
    a query or fetch sees its own namespace only, and ``delete_all`` empties one namespace.
    ``""`` (or ``None``) is the default namespace, stored and searched exactly as an index
    without namespaces.  Every named namespace lives in one second ``ShardSet``, the pool
    (same dimension, dtype, metric and devices; made by the first upsert into a named
    namespace, grown by doubling), which hands its rows out in pages (``pages``); a query
    there is the exact scan over the namespace's own pages (``ShardSet.search_pages``), so it
    costs what the namespace holds, not what the pool holds, and gives the scores, order and
    ties of an index holding that namespace alone.  A namespace exists while it holds a
    vector.  In a named namespace ``query_batch`` takes ``mode="auto"`` or ``"scan"``
    (``"mfma"`` / ``"mfma_masked"`` raise ``ValueError``) unless the index was made with
    ``paged_search="mfma"``: then ``query_batch`` there takes all four modes and hands them to
    the batched MFMA search over the namespace's pages (``ShardSet.search_pages(mode=...)``;
    ``"auto"`` scans under a metadata filter and otherwise follows the library's measured
    rule), with the scan's ids and score bits.  That needs an f16/bf16 index with
    ``filter="native"`` or ``"metric"`` (the pool gets the metric filter when the index has it);
    anything else raises ``ValueError`` at construction.  ``paged_search="scan"`` (default)
    changes nothing; ``query`` always scans.

    ``metadata_config={"indexed": ["field", ...]}`` (Pinecone's pod-index knob; default ``None``)
    keeps the named metadata fields as typed columns on the leader device (``metacolumns``: 9
    bytes per row and field), and a metadata filter over those fields becomes its bitmap in one
    kernel (``rc_meta_eval``) instead of a Python pass over every row.  Results never change:
    the bitmap is bit-identical to ``metafilter.build_bitmap``'s, and a filter that names another
    field, a field holding a value without a column encoding (a list, ``None``, ...: the field is
    demoted for the life of the object) or an operand without one is evaluated on the host as
    before.  ``metadata_index_stats()`` reports which path ran.  Anything but a dict with exactly
    the key ``"indexed"`` and a list of distinct non-empty names not starting with ``$`` raises
    ``ValueError``.

    ``max_top_k`` (default 256; anything outside [256, 10000] raises ``ValueError``) opts the
    index into deep top-k: ``query`` and ``query_batch`` then accept ``top_k <= max_top_k``.
    A ``top_k`` up to 256 takes the paths above, untouched; a larger one goes through the deep
    search (``ShardSet.search_deep`` / ``search_pages_deep``: one pass over the rows that keeps
    every score, then ``ceil(top_k / 256)`` selection rounds over the scores), in the default
    namespace and in named ones, with or without a metadata filter, under every dtype, metric
    and filter kind.  Its matches are those an exact scan able to hold ``top_k`` results would
    give: the first 256 are the ``top_k=256`` answer, scores and tie order included.  ``mode``
    is validated and otherwise ignored there.  With the default every message and exception
    is what it was.  (``sharded.ShardedIndex``, one process per GPU, has no deep search.)

    ``sparse_max_nnz=W`` (default 0 = off; an integer in [1, 1024]; ``metric="dotproduct"`` only,
    ``ValueError`` otherwise, as in Pinecone) makes the index sparse-dense: a record may carry
    ``sparse_values={"indices": [...], "values": [...]}`` (at most ``W`` distinct indices in
    [0, 2**32 - 2], finite values) beside its mandatory dense vector — in ``upsert``'s dict items
    and ``upsert_tensor(sparse_values=...)``; an upsert without them clears the id's entries —
    and ``query(..., sparse_vector=...)`` / ``query_batch(..., sparse_vectors=[...])`` (up to 1024
    entries each, whatever ``W``) score ``dense . dense + sparse . sparse``.  Such a query goes through the hybrid search
    (``ShardSet.search_hybrid`` / ``search_pages_hybrid``: the deep search with the sparse add
    kernel between its score pass and its selection) for every ``top_k``, with metadata filters,
    in named namespaces and over several shards; ``mode`` is validated and otherwise ignored.  A
    query without a sparse part (``None`` or an empty pair) takes the paths above, untouched.
    ``query(id=...)`` uses the id's stored dense and sparse parts.  ``fetch`` returns
    ``"sparse_values"`` for records that have them, and so do matches under
    ``include_values=True``; ``save`` / ``load`` keep them.  The store costs ``8 * W`` bytes per
    row slot of capacity on each shard.  With the default every path, message and snapshot byte
    is what it was.  (``sharded.ShardedIndex`` has no sparse values.)
    """

    def __init__(self, name: str, dimension: int = 768, metric: str = "cosine", dtype: str = "float32",
                 capacity: int = 1 << 20, device=None, shards: int | None = None, devices=None,
                 filter: str = "native", paged_search: str = "scan", metadata_config: dict | None = None,
                 max_top_k: int = _lib.RC_TOPK_MAX, sparse_max_nnz: int = 0):
        indexed = metacolumns.validate_config(metadata_config)
        sparse_max_nnz = sparsevalues.validate_width(sparse_max_nnz)
        if sparse_max_nnz and metric != "dotproduct":
            raise ValueError(f"sparse values need metric='dotproduct' (metric={metric!r}, sparse_max_nnz={sparse_max_nnz})")
        if isinstance(max_top_k, bool) or not isinstance(max_top_k, int) or not _lib.RC_TOPK_MAX <= max_top_k <= _lib.RC_DEEP_TOPK_MAX:
            raise ValueError(f"max_top_k must be an integer in [{_lib.RC_TOPK_MAX}, {_lib.RC_DEEP_TOPK_MAX}] (got {max_top_k!r})")
        if paged_search not in ("scan", "mfma"):
            raise ValueError(f"unknown paged_search {paged_search!r} (expected 'scan' or 'mfma')")
        if paged_search == "mfma" and (_lib.is_f8(dtype) or dtype in ("float32", "f32") or filter in ("i8", "f8")):
            raise ValueError("paged_search='mfma' runs the native f16 / bf16 kernels over pages: it needs dtype float16 or "
                             f"bfloat16 and filter 'native' or 'metric' (dtype={dtype!r}, filter={filter!r})")
        if metric not in _lib.METRICS:
            raise ValueError(f"unknown metric {metric!r} (expected one of {sorted(_lib.METRICS)})")
        if filter not in _lib.FILTERS:
            raise ValueError(f"unknown filter {filter!r} (expected one of {sorted(_lib.FILTERS)})")
        if metric != "cosine" and filter not in ("native", "metric"):
            raise ValueError(f"filter={filter!r} is cosine-only (metric={metric!r}); filter='metric' serves the other metrics")
        if filter == "metric" and (_lib.is_f8(dtype) or dtype in ("float32", "f32")):
            raise ValueError(f"filter='metric' reads stored f16 / bf16 rows: it needs dtype float16 or bfloat16 (dtype={dtype!r})")
        if _lib.is_f8(dtype) and filter == "i8":
            raise ValueError("filter='i8' is not available on a float8 index (its batched search is filter='f8')")
        if filter == "f8" and not _lib.is_f8(dtype):
            raise ValueError(f"filter='f8' reads stored float8 rows: it needs dtype='f8' (dtype={dtype!r})")
        if devices is None:
            devices = [device] * int(shards or 1)
        self.name = name
        self.dimension = int(dimension)
        self.metric = metric
        self.paged_search = paged_search
        self.max_top_k = max_top_k
        self.sparse_max_nnz = sparse_max_nnz
        n = len(devices)
        self._set = ShardSet(self.dimension, dtype=dtype, capacity_per_shard=max(1, -(-int(capacity) // n)),
                             devices=devices, metric=metric)
        if filter != "native":
            self._set.set_filter(filter)
        if sparse_max_nnz:
            self._set.sparse_enable(sparse_max_nnz)
        self._sparse: dict[str, tuple[np.ndarray, np.ndarray]] = {}  # id -> sparse values (default namespace)
        self._rows: dict[str, int] = {}
        self._ids: list[str] = []
        self._meta: dict[str, dict] = {}
        self._mu = threading.Lock()
        # values the last query(include_values=True) fetched, valid until the next upsert or delete: the
        # reference's search (retriever/utils.py:62-64) asks for values and its caller then
        # fetches the same ids (retriever/main.py:142) — each row leaves the GPU once
        self._gen = 0
        self._recent: tuple[int, dict[str, np.ndarray]] = (-1, {})
        # metadata-filter bitmaps, most recently used last: (canonical filter JSON, _gen) ->
        # (bitmap, eligible count); any upsert or delete bumps _gen, so stale entries can never be hit
        self._bitmaps: dict[tuple[str, int], tuple[np.ndarray, int]] = {}
        # named namespaces: their states by name, the pool they share (None until the first
        # upsert into one), the pool's page allocator and the page-table slots in use
        self._ns: dict[str, _Namespace] = {}
        self._pool: ShardSet | None = None
        self._alloc = pages.PageAllocator()
        self._free_slots: list[int] = []
        self._next_slot = 0
        # metadata columns (metadata_config): the host state both column sets share, the default
        # namespace's set (by global row) and the pool's (by pool row, made with the pool)
        self.metadata_config = None if indexed is None else {"indexed": list(indexed)}
        self._fields = None if indexed is None else metacolumns.FieldIndex(indexed)
        self._cols = metacolumns.Columns(len(indexed), self._set.capacity, self._set.device) if indexed else None
        self._pool_cols: "metacolumns.Columns | None" = None

    @property
    def _sparse_query_nnz(self) -> int:
        """Entries a query's sparse part may hold: the library's limit, whatever the records' ``sparse_max_nnz``; 0 when off."""
        return sparsevalues.MAX_NNZ if self.sparse_max_nnz else 0

    @property
    def shard_set(self) -> ShardSet:
        return self._set

    @property
    def pool(self) -> "ShardSet | None":
        """The ShardSet holding every named namespace (None before the first one)."""
        return self._pool

    @property
    def dtype(self) -> str:
        return self._set.dtype

    @property
    def capacity(self) -> int:
        return self._set.capacity

    @property
    def shard_devices(self) -> list[int]:
        """GPU of each shard (global row g lives on shard g % len(shard_devices))."""
        return list(self._set.devices)

    def __len__(self) -> int:
        return len(self._ids)

    def close(self) -> None:
        self._set.close()
        if self._pool is not None:
            self._pool.close()

    def _normalize_items(self, vectors: Iterable, sparse_out: dict | None = None) -> list[tuple[str, list[float], dict]]:
        """``sparse_out`` (a sparse-dense index): receives id -> the item's validated sparse values
        (``None`` for none); an item with ``"sparse_values"`` on any other index raises."""
        items: dict[str, tuple[str, list[float], dict]] = {}
        for v in vectors:
            if isinstance(v, dict):
                vid, vals, md = v["id"], v["values"], v.get("metadata") or {}
                if v.get("sparse_values") is not None or sparse_out is not None:
                    sp = sparsevalues.normalize(v.get("sparse_values"), self.sparse_max_nnz)
                    if sparse_out is not None and isinstance(vid, str):
                        sparse_out[vid] = sp
            else:
                v = tuple(v)
                if len(v) == 2:
                    (vid, vals), md = v, {}
                elif len(v) == 3:
                    vid, vals, md = v
                    md = md or {}
                else:
                    raise ValueError("vectors must be (id, values[, metadata]) tuples or dicts")
            if not isinstance(vid, str) or not vid:
                raise ValueError("vector id must be a non-empty string")
            # one row per id: a repeated id in one call keeps its LAST values (two
            # writes of one row slot in the same launch would interleave)
            items[vid] = (vid, _as_vector(vals, self.dimension), dict(md))
            if sparse_out is not None and not isinstance(v, dict):
                sparse_out[vid] = None  # (the last occurrence of an id wins, its sparse values included)
        return list(items.values())

    def _ensure_capacity(self, n_total: int) -> None:
        if n_total <= self._set.capacity:
            return
        per = self._set.capacity_per_shard
        need = -(-n_total // self._set.n)
        while per < need:
            per *= 2
        self._set.grow(per)

    def upsert(self, vectors: Sequence, namespace: str = "") -> dict:
        namespace = _namespace_name(namespace)
        by_id: dict | None = {} if self.sparse_max_nnz else None
        items = self._normalize_items(vectors, by_id)
        if not items:
            return {"upserted_count": 0}
        sp = None if by_id is None else [by_id[it[0]] for it in items]
        vecs = torch.tensor([it[1] for it in items], dtype=torch.float32)
        with self._mu:
            if namespace:
                self._ns_upsert_locked(namespace, items, lambda pool, rows: pool.upsert_rows(vecs, rows), sp)
            else:
                self._upsert_locked(items, vecs, sp)
        return {"upserted_count": len(items)}

    def _sparse_arg(self, sparse_values, n: int):
        """``upsert_tensor``'s ``sparse_values``: one entry (dict or ``None``) per id, validated; ``None``
        on an index without sparse values (where passing any raises)."""
        if sparse_values is None:
            return [None] * n if self.sparse_max_nnz else None
        sparse_values = list(sparse_values)
        if len(sparse_values) != n:
            raise ValueError("sparse_values and ids differ in length")
        sp = [sparsevalues.normalize(x, self.sparse_max_nnz) for x in sparse_values]
        return sp if self.sparse_max_nnz else None

    def upsert_tensor(self, ids: Sequence[str], vecs, metadata: Sequence[dict] | None = None, namespace: str = "",
                      sparse_values: Sequence | None = None) -> dict:
        """Batched upsert of device-resident vectors (the ingest path: embeddings never leave HBM).

        ``vecs``: f32 [len(ids), dimension] on a GPU, or a list of parts ``(positions,
        tensor)`` — the vectors of ``ids[positions]`` on whatever GPU produced them (an
        ``EmbedderPool`` batch): each goes straight to its shard's GPU.  Same semantics as
        ``upsert`` (overwrite by id, last occurrence wins).  ``sparse_values`` (a sparse-dense
        index): one ``{"indices", "values"}`` dict or ``None`` per id."""
        namespace = _namespace_name(namespace)
        sp_all = self._sparse_arg(sparse_values, len(ids))
        if isinstance(vecs, (list, tuple)):
            return self._upsert_parts(ids, vecs, metadata, namespace, sp_all)
        if vecs.dim() != 2 or vecs.shape[0] != len(ids) or vecs.shape[1] != self.dimension:
            raise ValueError("vecs must be [len(ids), dimension]")
        metadata = list(metadata) if metadata is not None else [{}] * len(ids)
        if len(metadata) != len(ids):
            raise ValueError("metadata and ids differ in length")
        last: dict[str, int] = {}
        for i, vid in enumerate(ids):
            if not isinstance(vid, str) or not vid:
                raise ValueError("vector id must be a non-empty string")
            last[vid] = i
        keep = list(last.values())
        if len(keep) != len(ids):
            vecs = vecs[torch.tensor(keep, dtype=torch.int64, device=vecs.device)]
        nonzero = (vecs != 0).any(dim=1).all()  # queued behind the producer of vecs; read below
        items = [(ids[i], None, dict(metadata[i] or {})) for i in keep]
        sp = None if sp_all is None else [sp_all[i] for i in keep]
        if not bool(nonzero):
            raise ValueError("Dense vectors must contain at least one non-zero value for the cosine metric")
        with self._mu:
            if namespace:
                self._ns_upsert_locked(namespace, items, lambda pool, rows: pool.upsert_rows(vecs, rows), sp)
            else:
                self._upsert_locked(items, vecs, sp)
        return {"upserted_count": len(items)}

    def _upsert_parts(self, ids, parts, metadata, namespace: str = "", sp_all=None) -> dict:
        metadata = list(metadata) if metadata is not None else [{}] * len(ids)
        if len(metadata) != len(ids):
            raise ValueError("metadata and ids differ in length")
        where: dict[int, tuple[int, int]] = {}  # position -> (part, offset)
        for pi, (pos, t) in enumerate(parts):
            pos = [int(p) for p in pos]
            if t.dim() != 2 or t.shape[0] != len(pos) or t.shape[1] != self.dimension:
                raise ValueError("each part needs vectors [len(positions), dimension]")
            for o, p in enumerate(pos):
                where[p] = (pi, o)
        if sorted(where) != list(range(len(ids))):
            raise ValueError("the parts must cover every position of ids exactly once")
        last: dict[str, int] = {}
        for i, vid in enumerate(ids):
            if not isinstance(vid, str) or not vid:
                raise ValueError("vector id must be a non-empty string")
            last[vid] = i
        keep = list(last.values())
        for _, t in parts:
            if t.shape[0] and not bool((t != 0).any(dim=1).all()):
                raise ValueError("Dense vectors must contain at least one non-zero value for the cosine metric")
        items = [(ids[i], None, dict(metadata[i] or {})) for i in keep]
        sp = None if sp_all is None else [sp_all[i] for i in keep]
        def split(rows):  # the parts as ShardSet.upsert_parts takes them: (global rows, vectors)
            sel = [[] for _ in parts]  # per part: (offset, global row) of the kept positions
            for i, r in zip(keep, rows):
                pi, o = where[i]
                sel[pi].append((o, r))
            out = []
            for (pos, t), lst in zip(parts, sel):
                if not lst:
                    continue
                offs = torch.tensor([o for o, _ in lst], dtype=torch.int64)
                v = t if len(lst) == t.shape[0] and offs.tolist() == list(range(t.shape[0])) else t[offs.to(t.device)]
                out.append((torch.tensor([r for _, r in lst], dtype=torch.int64), v))
            return out

        with self._mu:
            if namespace:
                self._ns_upsert_locked(namespace, items, lambda pool, rows: pool.upsert_parts(split(rows)), sp)
            else:
                rows = self._plan_rows(items)
                self._device_write(self._set.upsert_parts, split(rows))
                self._device_write(self._columns_write, self._cols, self._set, rows, items)
                self._device_write(self._sparse_write, self._set, rows, sp)
                self._commit_rows(items, rows, sp)
        return {"upserted_count": len(items)}

    # ------------------------------------------------------------ named namespaces --
    def _ensure_pool(self) -> ShardSet:
        if self._pool is None:
            per = POOL_INITIAL_PAGES * pages.PAGE_ROWS
            self._pool = ShardSet(self.dimension, dtype=self._set.dtype, capacity_per_shard=per,
                                  devices=list(self._set.devices), metric=self.metric)
            if self.paged_search == "mfma" and self._set.filter == "metric":  # else the pool stays native
                self._pool.set_filter("metric")
            if self.sparse_max_nnz:  # the pool's own store, by pool row; it grows with the pool
                self._pool.sparse_enable(self.sparse_max_nnz)
            self._alloc.set_capacity(per // pages.PAGE_ROWS)
            if self._cols is not None:  # the pool's metadata columns, by pool row; they grow with it
                self._pool_cols = metacolumns.Columns(self._cols.n_fields, self._pool.capacity, self._pool.device)
        return self._pool

    def _take_pages(self, count: int) -> list[int]:
        """``count`` pool pages, growing the pool (doubling, ``rc_sharded_grow``) if it is short."""
        pool = self._ensure_pool()
        if self._alloc.pages_short(count):
            per = self._alloc.capacity_needed(count, pool.capacity_per_shard)
            pool.grow(per)
            self._alloc.set_capacity(pool.capacity_per_shard // pages.PAGE_ROWS)
        return self._alloc.alloc(count)

    def _ns_rows(self, ns: _Namespace, positions, page_list=None) -> list[int]:
        """Pool rows of a namespace's positions."""
        sp = pages.span(self._set.n)
        pl = ns.pages if page_list is None else page_list
        return [pl[p // sp] * sp + p % sp for p in positions]

    def _ns_upsert_locked(self, name: str, items, write, sp=None) -> None:
        """``_upsert_locked`` in a named namespace: positions for the items (an existing id keeps
        its position), the pages the new length needs, the device write ``write(pool, pool
        rows)``, the page table if it gained a page, then the host maps.  If the write raises
        nothing is registered and the new pages go back to the free list; a namespace made by
        this call never comes to exist."""
        ns = self._ns.get(name)
        fresh = ns is None
        if fresh:
            ns = _Namespace(name, self._free_slots.pop() if self._free_slots else self._next_slot)
        pos, nxt = [], len(ns._ids)
        for vid, _, _ in items:
            p = ns._rows.get(vid)
            if p is None:
                p, nxt = nxt, nxt + 1
            pos.append(p)
        gained = self._take_pages(pages.pages_for(nxt, self._set.n) - len(ns.pages))
        page_list = ns.pages + gained
        try:
            rows = self._ns_rows(ns, pos, page_list)
            write(self._pool, rows)
            self._columns_write(self._pool_cols, self._pool, rows, items)
            self._sparse_write(self._pool, rows, sp)
            if gained:
                self._pool.set_pages(ns.slot, page_list)
        except BaseException:
            ns._gen += 1
            self._alloc.free(gained)
            if fresh:
                self._free_slots.append(ns.slot)
            elif gained:  # the table may be half replaced: back to the list the host holds
                self._pool.set_pages(ns.slot, ns.pages)
            raise
        ns.pages = page_list
        if fresh:
            self._ns[name] = ns
            if ns.slot == self._next_slot:
                self._next_slot += 1
        for (vid, _, md), p in zip(items, pos):
            if vid not in ns._rows:
                ns._rows[vid] = p
                ns._ids.append(vid)
            ns._meta[vid] = md
        self._sparse_commit(ns, items, sp)
        ns._gen += 1

    def _ns_drop_locked(self, ns: _Namespace) -> None:
        """The namespace holds nothing any more: its pages, its table and its slot are free."""
        self._pool.set_pages(ns.slot, [])
        self._alloc.free(ns.pages)
        self._free_slots.append(ns.slot)
        del self._ns[ns.name]

    def _ns_delete_rows_locked(self, ns: _Namespace, positions: list[int]) -> None:
        """``_delete_rows_locked`` on a namespace's positions (distinct, ascending): the same
        plan (position i is on shard i % n, as a global row is), the moves on pool rows, the
        host maps, then the pages past the new length go back to the free list."""
        if not positions:
            return
        n = len(ns._ids)
        src, dst = compaction.plan_compaction(n, positions, self._set.n)
        if src:
            try:
                self._pool.move_rows(self._ns_rows(ns, src), self._ns_rows(ns, dst))
                self._columns_move(self._pool_cols, self._ns_rows(ns, src), self._ns_rows(ns, dst))
                self._sparse_move(self._pool, ns, src, self._ns_rows(ns, dst))
            except BaseException:
                ns._gen += 1
                raise
        ids = ns._ids
        for p in positions:
            vid = ids[p]
            del ns._rows[vid]
            ns._meta.pop(vid, None)
            ns._sparse.pop(vid, None)
        for s, d in zip(src, dst):
            vid = ids[s]
            ids[d] = vid
            ns._rows[vid] = d
        del ids[n - len(positions):]
        ns._gen += 1
        if not ids:
            self._ns_drop_locked(ns)
            return
        keep = pages.pages_for(len(ids), self._set.n)
        if keep < len(ns.pages):
            gone, ns.pages = ns.pages[keep:], ns.pages[:keep]
            self._pool.set_pages(ns.slot, ns.pages)
            self._alloc.free(gone)

    def _plan_rows(self, items) -> list[int]:
        """Row of each (deduplicated) item: its existing row, or the next free rows; grows the
        shards if needed.  Registers nothing (see _commit_rows)."""
        rows, nxt = [], len(self._ids)
        for vid, _, _ in items:
            r = self._rows.get(vid)
            if r is None:
                r, nxt = nxt, nxt + 1
            rows.append(r)
        self._ensure_capacity(nxt)
        return rows

    def _commit_rows(self, items, rows, sp=None) -> None:
        for (vid, _, md), r in zip(items, rows):
            if vid not in self._rows:
                self._rows[vid] = r
                self._ids.append(vid)
            self._meta[vid] = md
        self._sparse_commit(self, items, sp)
        self._gen += 1

    # sparse values (sparse_max_nnz): the host keeps each id's, as it keeps metadata; the device store
    # is written where the metadata columns are and re-written where they move
    def _sparse_write(self, owner: ShardSet, rows, sp) -> None:
        """The store slots of the rows an upsert just wrote: ALL slots of every row (padding where
        an item has no sparse values), so a reused row shows nothing of its former owner."""
        if self.sparse_max_nnz:
            owner.sparse_write(rows, sp if sp is not None else [None] * len(rows))

    def _sparse_commit(self, st, items, sp) -> None:
        if not self.sparse_max_nnz:
            return
        for i, (vid, _, _) in enumerate(items):
            x = None if sp is None else sp[i]
            if x is None:
                st._sparse.pop(vid, None)  # an upsert without sparse values clears the id's entries
            else:
                st._sparse[vid] = x

    def _sparse_move(self, owner: ShardSet, st, src, dst_rows) -> None:
        """After a compaction's row moves (before the host maps change): the destination rows get
        the sparse values of the ids that moved there.  ``src``: rows / positions of ``st``."""
        if self.sparse_max_nnz and src:
            owner.sparse_write(dst_rows, [st._sparse.get(st._ids[r]) for r in src])

    def _device_write(self, fn, *args) -> None:
        """A shard write under the lock.  If it raises part-way (an earlier shard already
        overwrote the rows of existing ids), the values cached by the last query no longer
        match the device: invalidate them before re-raising, so fetch reads the device."""
        try:
            fn(*args)
        except BaseException:
            self._gen += 1
            raise

    def _columns_write(self, cols, owner: ShardSet, rows, items) -> None:
        """The metadata columns of the rows an upsert just wrote: ALL fields of every row (tag 0
        where a field is absent), so a reused row shows nothing of its former owner.  After the
        vector write, before the host maps are committed.  If it raises, the columns are marked
        invalid — every filter then takes the host path, a stale column never makes a bitmap —
        and the error propagates like a failed vector write."""
        fx = self._fields
        if cols is None or not fx.valid:
            return
        try:
            cols.ensure(owner.capacity)  # the vectors' capacity: the columns grow with it
            tags, vals = fx.encode([md for _, _, md in items])
            cols.write(rows, tags, vals)
        except BaseException:
            fx.valid = False
            raise

    def _columns_move(self, cols, src, dst) -> None:
        """The columns follow a compaction's (src, dst) plan (after ``move_rows`` succeeded)."""
        fx = self._fields
        if cols is None or not fx.valid:
            return
        try:
            cols.move(src, dst)
        except BaseException:
            fx.valid = False
            raise

    def metadata_index_stats(self) -> dict:
        """``{"indexed": the configured fields, "device": those still evaluated on the device,
        "demoted": {field: reason}, "valid": whether the device columns are in use, "device_evals" /
        "host_evals": bitmap cache misses by the path that built the bitmap}``.  Without
        ``metadata_config``: no fields, not valid, and both counters stay 0."""
        with self._mu:
            if self._fields is None:
                return {"indexed": [], "device": [], "demoted": {}, "valid": False, "device_evals": 0, "host_evals": 0}
            return self._fields.stats()

    def _upsert_locked(self, items, vecs: torch.Tensor, sp=None) -> None:
        # device write first: if it raises, no id is registered (no zero rows behind live ids)
        rows = self._plan_rows(items)
        self._device_write(self._set.upsert_rows, vecs, rows)
        self._device_write(self._columns_write, self._cols, self._set, rows, items)
        self._device_write(self._sparse_write, self._set, rows, sp)
        self._commit_rows(items, rows, sp)

    def delete(self, ids: Sequence[str] | None = None, delete_all: bool = False, namespace: str = "",
               filter: dict | None = None) -> dict:
        """Pinecone's ``delete``: remove the vectors named by ``ids``, or every vector whose
        metadata satisfies ``filter`` (``query``'s metadata filter), or all of them
        (``delete_all=True``).  Exactly one of the three selects (``ValueError`` otherwise; an
        empty ``filter`` selects nothing and does not count); unknown and repeated ids are
        ignored.  Returns ``{}``.

        The live rows stay dense (``compaction``): each deleted row below the new length is
        overwritten with a surviving row of the tail, so at most as many stored rows move as
        are deleted, no search kernel changes and unfiltered queries pay nothing.  Rows at or
        past the new length keep stale bytes that no search scores (they all stop at
        ``n_rows``); capacity never shrinks, and the next upserts reuse the freed rows.

        If the device move raises, no id is removed: surviving ids are intact (moves only
        write into rows of ids being deleted), but the ids being deleted may now hold another
        vector's values.  The cached values and bitmaps are invalidated and the error is
        re-raised; repeat the call."""
        self._delete(ids, delete_all, filter, namespace)
        return {}

    def _delete(self, ids, delete_all, flt, namespace: str = "") -> int:
        """``delete``'s body; returns how many vectors were removed (Pinecone's call reports
        nothing; the package's ``/delete_images`` route answers with the count)."""
        if flt is not None and not isinstance(flt, dict):
            raise ValueError("filter must be a dict (Pinecone metadata filter) or None")
        if isinstance(ids, (str, bytes)):
            raise ValueError("ids must be a list of ids, not one string")
        if (ids is not None) + bool(delete_all) + bool(flt) != 1:
            raise ValueError("delete needs exactly one of ids, delete_all=True or a non-empty filter")
        namespace = _namespace_name(namespace)
        if namespace:
            with self._mu:
                ns = self._ns.get(namespace)
                if ns is None:  # nothing there: Pinecone's delete in an unknown namespace is a no-op
                    return 0
                if delete_all:
                    n = len(ns._ids)
                    self._ns_drop_locked(ns)
                    return n
                if ids is not None:
                    pos = sorted({ns._rows[i] for i in ids if i in ns._rows})
                else:
                    bitmap, eligible = self._bitmap_locked(flt, ns)
                    bits = np.unpackbits(bitmap.view(np.uint8), bitorder="little")[:len(ns._ids)]
                    pos = np.flatnonzero(bits).tolist() if eligible else []
                self._ns_delete_rows_locked(ns, pos)
                return len(pos)
        with self._mu:
            if delete_all:
                n = len(self._ids)
                self._ids, self._rows, self._meta = [], {}, {}  # the stored rows are simply never searched again
                self._sparse = {}
                self._gen += 1
                return n
            if ids is not None:
                rows = sorted({self._rows[i] for i in ids if i in self._rows})
            else:
                bitmap, eligible = self._bitmap_locked(flt)
                bits = np.unpackbits(bitmap.view(np.uint8), bitorder="little")[:len(self._ids)]
                rows = np.flatnonzero(bits).tolist() if eligible else []
            self._delete_rows_locked(rows)
            return len(rows)

    def _delete_rows_locked(self, rows: list[int]) -> None:
        """rows: distinct live rows, ascending.  Plan, device moves, then the host maps in
        O(len(rows)), then a new generation (no cached bitmap or value can be hit again)."""
        if not rows:
            return
        n = len(self._ids)
        src, dst = compaction.plan_compaction(n, rows, self._set.n)
        if src:
            self._device_write(self._set.move_rows, src, dst)
            self._device_write(self._columns_move, self._cols, src, dst)
            self._device_write(self._sparse_move, self._set, self, src, dst)
        ids = self._ids
        for r in rows:
            vid = ids[r]
            del self._rows[vid]
            self._meta.pop(vid, None)
            self._sparse.pop(vid, None)
        for s, d in zip(src, dst):
            vid = ids[s]
            ids[d] = vid
            self._rows[vid] = d
        del ids[n - len(rows):]
        self._gen += 1

    def _bitmap_locked(self, flt, st=None) -> tuple[np.ndarray, int] | None:
        """The row-eligibility bitmap of a metadata filter and its eligible count (None for no
        filter: ``None`` or ``{}``).  Cached per (canonical filter, generation).  ``st``: a named
        namespace's state (the bitmap is then over its positions, the cache its own)."""
        if st is None:
            st = self
        if flt is None:
            return None
        if not isinstance(flt, dict):
            raise ValueError("filter must be a dict (Pinecone metadata filter) or None")
        if not flt:
            return None
        key = (metafilter.canonical(flt), st._gen)
        cache = st._bitmaps
        hit = cache.pop(key, None)
        if hit is None:
            hit = self._build_bitmap_locked(flt, st)
            for old in [k for k in cache if k[1] != st._gen]:
                del cache[old]
            while len(cache) >= BITMAP_CACHE_ENTRIES:
                del cache[next(iter(cache))]  # least recently used
        cache[key] = hit  # (re)inserted last = most recently used
        return hit

    def _build_bitmap_locked(self, flt, st) -> tuple[np.ndarray, int]:
        """A bitmap cache miss.  With valid metadata columns and a filter that compiles to a
        program over them (``metacolumns.compile_program``), ``rc_meta_eval`` on the leader's
        current stream and one copy back; otherwise — and always without ``metadata_config`` —
        ``metafilter.build_bitmap`` over the host's metadata.  The two give the same bits."""
        pred = metafilter.compile_filter(flt)
        fx = self._fields
        if fx is None:
            return metafilter.build_bitmap(pred, st._ids, st._meta)
        n = len(st._ids)
        cols = self._cols if st is self else self._pool_cols
        if cols is not None and fx.valid and n >= metacolumns.DEVICE_MIN_ROWS:
            program = fx.program(flt)
            if program is not None:
                if st is self:
                    hit = cols.eval(program, n)
                else:
                    hit = cols.eval(program, n, pages=st.pages, span=pages.span(self._set.n))
                fx.device_evals += 1
                return hit
        fx.host_evals += 1
        return metafilter.build_bitmap(pred, st._ids, st._meta)

    def query(self, vector=None, top_k: int = 10, include_values: bool = False, include_metadata: bool = False,
              id: str | None = None, namespace: str = "", filter: dict | None = None, sparse_vector: dict | None = None,
              **_: Any) -> dict:
        """``filter``: a Pinecone-style metadata filter (``metafilter``); ``None`` / ``{}`` = no
        filter.  Not the constructor's ``filter`` (the filter-GEMM kind).  ``sparse_vector`` (a
        sparse-dense index): the query's sparse part; the score is then ``dense . dense + sparse .
        sparse`` (the hybrid search, for every ``top_k``).  ``id=``: the id's stored dense and
        sparse parts."""
        if vector is None and id is None:
            raise ValueError("query needs a vector or an id")
        sp = sparsevalues.normalize(sparse_vector, self._sparse_query_nnz, "sparse_vector")
        if isinstance(top_k, bool) or int(top_k) != top_k or top_k < 1:
            raise ValueError("top_k must be a positive integer")
        top_k = int(top_k)
        if top_k > self.max_top_k:
            raise ValueError(f"top_k must be <= {self.max_top_k}")
        deep = top_k > _lib.RC_TOPK_MAX  # only with max_top_k: the deep search, through _query_locked
        namespace = _namespace_name(namespace)
        if namespace:
            with self._mu:
                ns = self._ns.get(namespace)
                if ns is None:  # no such namespace: no device work
                    return {"matches": [], "namespace": namespace}
                if vector is None:
                    p = ns._rows.get(id)
                    if p is None:
                        return {"matches": [], "namespace": namespace}
                    vector = self._pool.fetch_rows(self._ns_rows(ns, [p]))[0]
                    sp = ns._sparse.get(id)
                q = _as_vector_np(vector, self.dimension)
                bm = self._bitmap_locked(filter, ns)
                if sp is not None:
                    res = self._query_locked(torch.from_numpy(q), top_k, include_values, include_metadata, "scan", bm, ns, [sp])[0]
                elif deep:
                    res = self._query_locked(torch.from_numpy(q), top_k, include_values, include_metadata, "scan", bm, ns)[0]
                else:
                    res = self._query_host_locked(q, top_k, include_values, include_metadata, bm, ns)[0]
            return {"matches": res, "namespace": namespace}
        with self._mu:
            if vector is None:
                r = self._rows.get(id)
                if r is None:
                    return {"matches": [], "namespace": namespace}
                vector = self._set.fetch_rows([r])[0]
                sp = self._sparse.get(id)
            q = _as_vector_np(vector, self.dimension)
            bm = self._bitmap_locked(filter)
            if sp is not None:
                res = self._query_locked(torch.from_numpy(q), top_k, include_values, include_metadata, "scan", bm, None, [sp])[0]
            elif deep:
                res = self._query_locked(torch.from_numpy(q), top_k, include_values, include_metadata, "scan", bm)[0]
            else:
                res = self._query_host_locked(q, top_k, include_values, include_metadata, bm)[0]
        return {"matches": res, "namespace": namespace}

    def query_batch(self, vectors, top_k: int = 10, include_values: bool = False,
                    include_metadata: bool = False, mode: str = "auto", filter: dict | None = None,
                    namespace: str = "", sparse_vectors: Sequence | None = None) -> list[dict]:
        """Batched form of ``query`` (f16/bf16 shards run the MFMA path for >= 8 queries).
        ``filter``: one metadata filter for the whole batch (see ``query``); with ``mode="auto"``
        a filtered batch takes the MFMA path at an eligible share of at least
        ``MASKED_MFMA_MIN_SHARE``, and below it the MFMA path with the mask inside the filter
        GEMM (``mode="mfma_masked"``) where ``_masked_mode``'s measured rule allows; otherwise
        the masked scan.  ``namespace``: a named namespace scans its own pages (``mode`` "auto" or
        "scan" there; "mfma" / "mfma_masked" raise ``ValueError``), unless the index has
        ``paged_search="mfma"``: then all four modes go down to the batched MFMA search over the
        namespace's pages ("auto" scans under a metadata filter, and otherwise follows the
        library's rule).  ``sparse_vectors`` (a sparse-dense index): one sparse part (or ``None``)
        per query; if any query has one, the whole batch takes the hybrid search (``mode`` is
        validated and otherwise ignored)."""
        if top_k < 1 or top_k > self.max_top_k:
            raise ValueError(f"top_k must be in [1, {self.max_top_k}]")
        sp = None
        if sparse_vectors is not None:
            sp = [sparsevalues.normalize(x, self._sparse_query_nnz, "sparse_vector") for x in sparse_vectors]
            if all(x is None for x in sp):
                sp = None
        if isinstance(vectors, torch.Tensor):
            q = vectors.to(torch.float32)
            if q.dim() != 2 or q.shape[1] != self.dimension:
                raise ValueError("queries must be [n, dimension]")
        else:
            q = torch.tensor([_as_vector(v, self.dimension) for v in vectors], dtype=torch.float32)
        if sp is not None and len(sp) != q.shape[0]:
            raise ValueError("sparse_vectors and vectors differ in length")
        namespace = _namespace_name(namespace)
        if namespace:
            if mode not in _lib.SEARCH_MODES:
                raise ValueError(f"unknown search mode {mode!r}")
            if self.paged_search != "mfma":
                if mode not in ("auto", "scan"):
                    raise ValueError(f"mode={mode!r} is not available in a named namespace of this index (use 'auto' or "
                                     "'scan'): the batched MFMA search over pages is enabled with Index(..., paged_search='mfma')")
                mode = "scan"
            with self._mu:
                ns = self._ns.get(namespace)
                if ns is None:
                    res = [[] for _ in range(q.shape[0])]
                else:
                    res = self._query_locked(q, top_k, include_values, include_metadata, mode, self._bitmap_locked(filter, ns), ns, sp)
            return [{"matches": m, "namespace": namespace} for m in res]
        with self._mu:
            res = self._query_locked(q, top_k, include_values, include_metadata, mode, self._bitmap_locked(filter), None, sp)
        return [{"matches": m, "namespace": ""} for m in res]

    def _masked_mode(self, mode: str, nq: int, n: int, eligible: int, k: int = 10) -> str:
        """The library's "auto" scans whenever a mask is given (it does not know the eligible
        share); this layer does, and asks for MFMA when the unmasked conditions hold (>= 8
        queries, >= 64k rows per shard, an f16/bf16 index or the int8 filter copy; a float8
        index with the "f8" filter has the library's own corner for that kind, in passes of the
        masked scan) and the share reaches MASKED_MFMA_MIN_SHARE.  A non-cosine index scans unless
        its filter is "metric"; then the size rule is that filter's own (>= 16 queries, or >= 8
        over >= 2^28 bytes of rows per shard: measured unmasked, where 8 queries over fewer rows
        are behind the scan) and the share is the same constant (measured for cosine; under a
        metric it is unmeasured, and conservative: the competing masked scan takes one query per
        pass there).  Below that share a cosine f16/bf16 index with the native filter gets
        "mfma_masked" (the mask inside the filter GEMM) for >= MASK_FILTER_MIN_QUERIES queries, a
        share >= MASK_FILTER_MIN_SHARE and MASK_FILTER_MIN_ROWS .. MASK_FILTER_MAX_ROWS rows per
        shard, and above MASK_FILTER_LARGE_ROWS rows per shard only for >=
        MASK_FILTER_LARGE_MIN_QUERIES queries or a share >= MASK_FILTER_LARGE_MIN_SHARE: where it
        measured at least 2x ahead of the masked scan (f16; bf16 runs the same kernels at the
        same MFMA rate).  Everything else scans."""
        if mode != "auto":
            return mode
        if self.metric != "cosine" and self._set.filter != "metric":  # no batched path for this index
            return "scan"
        per_shard = n // self._set.n
        if _lib.is_f8(self._set.dtype):
            if self._set.filter != "f8":
                return "scan"
            ld = self._set.ld
            qb = 1 if k > 64 else 4 if ld <= 256 else 2 if ld <= 512 else 1  # the masked scan's queries per pass
            passes = -(-nq // qb)
            size_ok = (passes >= 16 and per_shard >= 131072) or (passes >= 8 and per_shard * ld >= 1 << 28)
        elif self.metric != "cosine":  # the "metric" filter's corner, as the library's unmasked "auto"
            size_ok = per_shard >= 65536 and (nq >= 16 or (nq >= 8 and per_shard * self._set.ld * 2 >= 1 << 28))
        else:
            mfma_ok = self._set.dtype not in ("float32", "f32") or self._set.filter == "i8"
            size_ok = mfma_ok and nq >= 8 and per_shard >= 65536
        if size_ok and eligible >= MASKED_MFMA_MIN_SHARE * n:
            return "mfma"
        # below that share: the mask inside the filter GEMM, where it was measured 2x ahead of the
        # masked scan (the MASK_FILTER_* constants' comment).  Measured on a cosine f16 index with
        # the native filter: the int8 / float8 filters and the metric forms have tested MASKED
        # kernels and no timing, so they scan.
        native_cosine = self.metric == "cosine" and self._set.filter in ("native", "metric") and not _lib.is_f8(self._set.dtype)
        in_box = (nq >= MASK_FILTER_MIN_QUERIES and MASK_FILTER_MIN_ROWS <= per_shard <= MASK_FILTER_MAX_ROWS and
                  eligible >= MASK_FILTER_MIN_SHARE * n)
        if per_shard > MASK_FILTER_LARGE_ROWS:
            in_box = in_box and (nq >= MASK_FILTER_LARGE_MIN_QUERIES or eligible >= MASK_FILTER_LARGE_MIN_SHARE * n)
        if size_ok and native_cosine and in_box:
            return "mfma_masked"
        return "scan"

    def _query_locked(self, q: torch.Tensor, k: int, include_values: bool, include_metadata: bool,
                      mode: str = "auto", bitmap=None, ns: _Namespace | None = None, sparse=None) -> list[list[dict]]:
        """``ns``: a named namespace's state — the paged search over its pages (``mode`` as
        ``query_batch`` resolved it: "scan" unless the index has ``paged_search="mfma"``); the rows
        that come back are its positions, mapped to pool rows where values are fetched.
        ``sparse``: the queries' sparse parts (a sparse-dense index) — the hybrid search, one path
        for every ``k``, whatever the mode, the filter kind or the mask's share."""
        st = self if ns is None else ns
        n = len(st._ids)
        if n == 0 or q.shape[0] == 0:
            return [[] for _ in range(q.shape[0])]
        if bitmap is not None and bitmap[1] == 0:  # nothing is eligible: no device work
            return [[] for _ in range(q.shape[0])]
        if sparse is not None:
            if mode not in _lib.SEARCH_MODES:
                raise ValueError(f"unknown search mode {mode!r}")
            mask = None if bitmap is None else bitmap[0]
            if ns is not None:
                scores, rows = self._pool.search_pages_hybrid(q, k, ns.slot, n, sparse, mask=mask)
            else:
                scores, rows = self._set.search_hybrid(q, k, n, sparse, mask=mask)
        elif k > _lib.RC_TOPK_MAX:  # deep top-k (max_top_k): one path whatever the mode, the filter kind or the mask's share
            if mode not in _lib.SEARCH_MODES:
                raise ValueError(f"unknown search mode {mode!r}")
            mask = None if bitmap is None else bitmap[0]
            if ns is not None:
                scores, rows = self._pool.search_pages_deep(q, k, ns.slot, n, mask=mask)
            else:
                scores, rows = self._set.search_deep(q, k, n, mask=mask)
        elif ns is not None:
            # (under a metadata filter the library's "auto" scans: the masked paged forms are unmeasured)
            scores, rows = self._pool.search_pages(q, k, ns.slot, n, mask=None if bitmap is None else bitmap[0], mode=mode)
        elif bitmap is None:
            scores, rows = self._set.search(q, k, n, mode=mode)
        else:
            if mode not in _lib.SEARCH_MODES:
                raise ValueError(f"unknown search mode {mode!r}")
            scores, rows = self._set.search(q, k, n, mode=self._masked_mode(mode, q.shape[0], n, bitmap[1], k),
                                            mask=bitmap[0])
        scores = scores.cpu().numpy()
        if self.metric == "euclidean":  # the library's -||q - v||^2 (descending) as Pinecone's squared distance
            scores = np.maximum(np.float32(0.0), -scores)
        scores = scores.tolist()
        rows = rows.cpu().tolist()
        out = []
        recent: dict[str, np.ndarray] = {}
        for sq, rq in zip(scores, rows):
            sel = [(s, r) for s, r in zip(sq, rq) if r >= 0]
            vals = None
            if include_values and sel:
                if ns is None:
                    vals = self._set.fetch_rows([r for _, r in sel]).numpy()
                else:
                    vals = self._pool.fetch_rows(self._ns_rows(ns, [r for _, r in sel])).numpy()
            if vals is not None:
                recent.update((st._ids[r], v) for (_, r), v in zip(sel, vals))
            matches = []
            for j, (s, r) in enumerate(sel):
                vid = st._ids[r]
                m = Record(vals[j], id=vid, score=float(s)) if include_values else {"id": vid, "score": float(s)}
                if include_values and vid in st._sparse:
                    dict.__setitem__(m, "sparse_values", sparsevalues.to_dict(st._sparse[vid]))
                if include_metadata:
                    dict.__setitem__(m, "metadata", dict(st._meta.get(vid, {})))
                matches.append(m)
            out.append(matches)
        if include_values:
            st._recent = (st._gen, recent)
        return out

    def _query_host_locked(self, q: np.ndarray, k: int, include_values: bool, include_metadata: bool,
                           bitmap=None, ns: _Namespace | None = None) -> list[list[dict]]:
        """The request path (a query or a few): ``ShardSet.query_host``, one library call, the
        lists and (include_values) the matched rows' values come back together.  ``ns``: a named
        namespace's state (``ShardSet.query_host_pages`` on the pool; the rows are positions)."""
        st = self if ns is None else ns
        n = len(st._ids)
        if n == 0 or (bitmap is not None and bitmap[1] == 0):  # (a filter nothing satisfies: no device work)
            return [[] for _ in range(q.shape[0])]
        if ns is not None:
            sc, rw, val = self._pool.query_host_pages(q, k, ns.slot, n, include_values,
                                                      mask=None if bitmap is None else bitmap[0])
        elif bitmap is None:
            sc, rw, val = self._set.query_host(q, k, n, include_values)
        else:
            sc, rw, val = self._set.query_host(q, k, n, include_values, mask=bitmap[0])
        out = []
        recent: dict[str, np.ndarray] = {}
        ids, meta = st._ids, st._meta
        for qi in range(q.shape[0]):
            rows = rw[qi].tolist()
            live = k - rows.count(-1)  # the lists are sorted: empty slots (-1) come last
            if self.metric == "euclidean":  # as in _query_locked
                scores = np.maximum(np.float32(0.0), -sc[qi, :live]).tolist()
            else:
                scores = sc[qi, :live].tolist()
            if include_values:
                # the reused host buffer is copied once (one memcpy); each match keeps its row as f32
                # and builds the Python list only if read (Record)
                vals = val[qi, :live].copy()
                matches = []
                for j in range(live):
                    vid = ids[rows[j]]
                    m = Record(vals[j], id=vid, score=scores[j])
                    if vid in st._sparse:
                        dict.__setitem__(m, "sparse_values", sparsevalues.to_dict(st._sparse[vid]))
                    recent[vid] = vals[j]
                    if include_metadata:
                        dict.__setitem__(m, "metadata", dict(meta.get(vid, {})))
                    matches.append(m)
            else:
                matches = [{"id": ids[r], "score": s} for s, r in zip(scores, rows[:live])]
                if include_metadata:
                    for m in matches:
                        m["metadata"] = dict(meta.get(m["id"], {}))
            out.append(matches)
        if include_values:
            st._recent = (st._gen, recent)
        return out

    def fetch(self, ids: Sequence[str], namespace: str = "") -> dict:
        namespace = _namespace_name(namespace)
        with self._mu:
            # a named namespace has its own ids, rows (positions) and cache of recently queried
            # values: nothing fetched in one namespace can be served in another
            st = self._ns.get(namespace) if namespace else self
            vectors = {}
            if st is None:
                return {"vectors": vectors, "namespace": namespace}
            found = [(i, st._rows[i]) for i in ids if i in st._rows]
            gen, recent = st._recent
            if found and gen == st._gen and all(i in recent for i, _ in found):
                vals = [recent[i] for i, _ in found]  # fetched by the query just before: no second device read
            elif found and st is self:
                vals = self._set.fetch_rows([r for _, r in found]).numpy()
            elif found:
                vals = self._pool.fetch_rows(self._ns_rows(st, [r for _, r in found])).numpy()
            if found:
                for (vid, _), v in zip(found, vals):
                    rec = Record(v, id=vid)  # "values" becomes a list when read (retriever/main.py reads metadata)
                    if vid in st._sparse:
                        dict.__setitem__(rec, "sparse_values", sparsevalues.to_dict(st._sparse[vid]))
                    dict.__setitem__(rec, "metadata", dict(st._meta.get(vid, {})))
                    vectors[vid] = rec
        return {"vectors": vectors, "namespace": namespace}

    # ---------------------------------------------------------- persistence --
    # Pinecone keeps an index durable server-side (the reference only opens it by
    # name, ingesting/utils.py:23-38); the in-HBM index is saved to a directory:
    # manifest.json (name, dimension, dtype, ids in row order, metadata) +
    # rows.npy (raw stored bytes in GLOBAL row order, exactly what search scores;
    # independent of the shard count) + norms.npy.  That is format 1, and what an index without
    # named namespaces writes.  With named namespaces the manifest is format 2: it also lists
    # them ("namespaces": name, count, ids in position order, metadata) and each has its own
    # ns<i>_rows.npy / ns<i>_norms.npy, raw stored rows in POSITION order — independent of the
    # pages the namespace happened to hold and of the shard count.
    SNAPSHOT_FORMAT = 1
    SNAPSHOT_FORMAT_NAMESPACES = 2

    def save(self, path: str) -> None:
        import numpy as np

        with self._mu:
            os.makedirs(path, exist_ok=True)
            n = len(self._ids)
            rows, norms = self._set.export_rows(n)
            np.save(os.path.join(path, "rows.npy"), rows)
            np.save(os.path.join(path, "norms.npy"), norms)
            self._save_sparse(path, "", self)
            spaces = []
            for i, ns in enumerate(self._ns.values()):
                cnt = len(ns._ids)
                el = _lib.dtype_bytes(self._set.dtype)
                nrows = np.zeros((cnt, self._set.ld * el), dtype=np.uint8)
                nnorms = np.zeros((cnt,), dtype=np.float32)
                for pos0, row0, m in pages.row_runs(ns.pages, cnt, self._set.n):  # runs of consecutive pages: one export each
                    nrows[pos0:pos0 + m], nnorms[pos0:pos0 + m] = self._pool.export_run(row0, m)
                np.save(os.path.join(path, f"ns{i}_rows.npy"), nrows)
                np.save(os.path.join(path, f"ns{i}_norms.npy"), nnorms)
                self._save_sparse(path, f"ns{i}_", ns)
                spaces.append({"name": ns.name, "count": cnt, "ids": list(ns._ids),
                               "metadata": {v: ns._meta.get(v, {}) for v in ns._ids}})
            manifest = {"format": self.SNAPSHOT_FORMAT_NAMESPACES if spaces else self.SNAPSHOT_FORMAT,
                        "name": self.name, "dimension": self.dimension,
                        "metric": self.metric, "dtype": self._set.dtype, "ld": self._set.ld, "count": n,
                        "capacity": self._set.capacity, "filter": self._set.filter,
                        "ids": list(self._ids), "metadata": {i: self._meta.get(i, {}) for i in self._ids}}
            if spaces:
                manifest["namespaces"] = spaces
            if self.metadata_config is not None:  # only then: every other manifest stays byte for byte what it was
                manifest["metadata_config"] = {"indexed": list(self.metadata_config["indexed"])}
            if self.sparse_max_nnz:  # likewise only then
                manifest["sparse_max_nnz"] = self.sparse_max_nnz
            tmp = os.path.join(path, "manifest.json.tmp")
            with open(tmp, "w") as f:
                json.dump(manifest, f)
            os.replace(tmp, os.path.join(path, "manifest.json"))  # the manifest lands last

    def _save_sparse(self, path: str, prefix: str, st) -> None:
        """A sparse-dense index only: the sparse values of ``st``'s ids in row (position) order as CSR,
        ``<prefix>sparse_off.npy`` int64 [count + 1], ``_idx.npy`` uint32, ``_val.npy`` float32."""
        if not self.sparse_max_nnz:
            return
        off, idx, val = sparsevalues.csr([st._sparse.get(vid) for vid in st._ids])
        total = int(off[-1])
        np.save(os.path.join(path, prefix + "sparse_off.npy"), off)
        np.save(os.path.join(path, prefix + "sparse_idx.npy"), idx[:total])
        np.save(os.path.join(path, prefix + "sparse_val.npy"), val[:total])

    @staticmethod
    def _load_sparse(path: str, prefix: str, count: int, width: int) -> list:
        off = np.load(os.path.join(path, prefix + "sparse_off.npy"), allow_pickle=False)
        idx = np.load(os.path.join(path, prefix + "sparse_idx.npy"), allow_pickle=False)
        val = np.load(os.path.join(path, prefix + "sparse_val.npy"), allow_pickle=False)
        if off.shape != (count + 1,) or off[0] != 0 or (np.diff(off) < 0).any() or idx.shape != (int(off[-1]),) or val.shape != idx.shape:
            raise ValueError("snapshot files disagree on the sparse values")
        out = []
        for i in range(count):
            a, b = int(off[i]), int(off[i + 1])
            out.append(sparsevalues.normalize({"indices": idx[a:b].tolist(), "values": val[a:b].tolist()}, width))
        return out

    @classmethod
    def load(cls, path: str, capacity: int | None = None, device=None, shards: int | None = None,
             devices=None, filter: str | None = None, paged_search: str = "scan",
             metadata_config: dict | None = None, max_top_k: int = _lib.RC_TOPK_MAX) -> "Index":
        """``metadata_config=None`` means the snapshot's own (none, if it was saved without one);
        the columns and string dictionaries are rebuilt from the loaded metadata.  ``max_top_k``
        is the loaded object's (the constructor's; a snapshot does not record it)."""
        import numpy as np

        with open(os.path.join(path, "manifest.json")) as f:
            man = json.load(f)
        if man.get("format") not in (cls.SNAPSHOT_FORMAT, cls.SNAPSHOT_FORMAT_NAMESPACES):
            raise ValueError(f"unsupported snapshot format {man.get('format')!r}")
        n = int(man["count"])
        idx = cls(man["name"], dimension=man["dimension"], metric=man["metric"], dtype=man["dtype"],
                  capacity=max(int(capacity or man.get("capacity", 0)), n, 1), device=device, shards=shards,
                  devices=devices, filter=filter or man.get("filter", "native"), paged_search=paged_search,
                  metadata_config=metadata_config if metadata_config is not None else man.get("metadata_config"),
                  max_top_k=max_top_k, **({"sparse_max_nnz": int(man["sparse_max_nnz"])} if "sparse_max_nnz" in man else {}))
        width = idx.sparse_max_nnz
        if idx._set.ld != man["ld"]:
            raise ValueError("snapshot row layout does not match this build")
        rows = np.load(os.path.join(path, "rows.npy"), allow_pickle=False)
        norms = np.load(os.path.join(path, "norms.npy"), allow_pickle=False)
        if rows.shape[0] != n or norms.shape[0] != n or len(man["ids"]) != n:
            raise ValueError("snapshot files disagree on the vector count")
        if n:
            idx._set.import_rows(rows, norms)
        idx._ids = list(man["ids"])
        idx._rows = {vid: r for r, vid in enumerate(idx._ids)}
        idx._meta = {vid: dict(man["metadata"].get(vid, {})) for vid in idx._ids}
        if n:
            with idx._mu:
                idx._columns_write(idx._cols, idx._set, list(range(n)), [(vid, None, idx._meta[vid]) for vid in idx._ids])
        if n and width:
            sp = cls._load_sparse(path, "", n, width)
            with idx._mu:
                idx._sparse_write(idx._set, list(range(n)), sp)
                idx._sparse_commit(idx, [(vid, None, None) for vid in idx._ids], sp)
        for i, sp in enumerate(man.get("namespaces", [])):
            cnt = int(sp["count"])
            nrows = np.load(os.path.join(path, f"ns{i}_rows.npy"), allow_pickle=False)
            nnorms = np.load(os.path.join(path, f"ns{i}_norms.npy"), allow_pickle=False)
            if nrows.shape[0] != cnt or nnorms.shape[0] != cnt or len(sp["ids"]) != cnt or not sp["name"] or cnt == 0:
                raise ValueError("snapshot files disagree on a namespace")
            items = [(vid, None, dict(sp["metadata"].get(vid, {}))) for vid in sp["ids"]]

            def write(pool, rows, nrows=nrows, nnorms=nnorms):  # rows: the pool rows of positions 0 .. cnt - 1
                r0 = 0
                while r0 < len(rows):  # runs of consecutive pool rows (whole pages but the last)
                    r1 = r0 + 1
                    while r1 < len(rows) and rows[r1] == rows[r1 - 1] + 1:
                        r1 += 1
                    pool.import_run(rows[r0], nrows[r0:r1], nnorms[r0:r1])
                    r0 = r1

            with idx._mu:
                idx._ns_upsert_locked(sp["name"], items, write, cls._load_sparse(path, f"ns{i}_", cnt, width) if width else None)
        return idx

    def describe_index_stats(self) -> dict:
        with self._mu:
            spaces = {"": {"vector_count": len(self._ids)}}
            spaces.update((name, {"vector_count": len(ns._ids)}) for name, ns in self._ns.items())
        return {"dimension": self.dimension, "index_fullness": len(self._ids) / self._set.capacity,
                "total_vector_count": sum(v["vector_count"] for v in spaces.values()), "namespaces": spaces,
                "shards": self._set.n}
