"""Sparse values of sparse-dense records and queries (Pinecone's ``sparse_values`` /
``sparse_vector``): validation, the float32 model of the device's sparse term, and the
client-side convex weighting.  Pure Python + numpy: nothing here touches a device.

A sparse vector is ``{"indices": [...], "values": [...]}``: distinct integer indices in
[0, 2**32 - 2] (2**32 - 1 is the store's padding), finite float values, the same length, at most
``max_nnz`` entries.  ``None`` and an empty pair both mean "none".  The normal form every other
module sees is ``(indices uint32 [nnz], values float32 [nnz])`` sorted ascending by index, or
``None``.
"""
from __future__ import annotations

import numpy as np

MAX_NNZ = 1024  # RC_SPARSE_MAX_NNZ: the widest store and the longest query
PAD = 0xFFFFFFFF  # the store's padding index: no record or query may carry it


def validate_width(width) -> int:
    """``Index(sparse_max_nnz=...)``: 0 (off) or an integer in [1, MAX_NNZ]."""
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or not 0 <= int(width) <= MAX_NNZ:
        raise ValueError(f"sparse_max_nnz must be 0 (off) or an integer in [1, {MAX_NNZ}] (got {width!r})")
    return int(width)


def normalize(sparse, max_nnz: int, what: str = "sparse_values"):
    """The normal form of one sparse vector, or ``None`` for none; ``ValueError`` for anything
    that is not a sparse vector of at most ``max_nnz`` entries."""
    if sparse is None:
        return None
    if isinstance(sparse, tuple) and len(sparse) == 2 and isinstance(sparse[0], np.ndarray):  # already normal (trusted: made here)
        return sparse if sparse[0].size else None
    if not isinstance(sparse, dict) or set(sparse) != {"indices", "values"}:
        raise ValueError(f"{what} must be a dict with exactly the keys 'indices' and 'values'")
    ind, val = sparse["indices"], sparse["values"]
    try:
        n_i, n_v = len(ind), len(val)
    except TypeError:
        raise ValueError(f"{what}: indices and values must be sequences") from None
    if n_i != n_v:
        raise ValueError(f"{what}: indices and values differ in length ({n_i} != {n_v})")
    if n_i == 0:
        return None
    if max_nnz <= 0:
        raise ValueError(f"{what}: this index holds no sparse values (make it with sparse_max_nnz > 0)")
    if n_i > max_nnz:
        raise ValueError(f"{what}: {n_i} entries exceed the limit of {max_nnz}")
    idx = np.empty(n_i, dtype=np.uint32)
    for j, i in enumerate(ind.tolist() if isinstance(ind, np.ndarray) else ind):
        if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= int(i) < PAD:
            raise ValueError(f"{what}: indices must be integers in [0, 2**32 - 2] (got {i!r})")
        idx[j] = int(i)
    try:
        v64 = np.asarray(val, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: values must be numbers") from None
    if v64.shape[0] != n_i or any(isinstance(v, (bool, str)) for v in (val.tolist() if isinstance(val, np.ndarray) else val)):
        raise ValueError(f"{what}: values must be numbers")
    with np.errstate(over="ignore"):
        v = v64.astype(np.float32)
    if not np.isfinite(v).all():
        raise ValueError(f"{what}: values must be finite float32 numbers")
    order = np.argsort(idx, kind="stable")
    idx, v = idx[order], v[order]
    if n_i > 1 and bool((idx[1:] == idx[:-1]).any()):
        raise ValueError(f"{what}: indices must be distinct")
    return np.ascontiguousarray(idx), np.ascontiguousarray(v)


def to_dict(sp) -> dict:
    """A normal form as Pinecone's dict (ascending indices, Python ints and floats)."""
    return {"indices": [int(i) for i in sp[0]], "values": [float(x) for x in sp[1]]}


def csr(sparse_list, offset_dtype=np.int64):
    """A list of normal forms (``None`` = no entries) as host CSR ``(off [n + 1], idx uint32,
    val float32)``, C-contiguous, never zero-length buffers' null pointers."""
    off = np.zeros(len(sparse_list) + 1, dtype=offset_dtype)
    for i, sp in enumerate(sparse_list):
        off[i + 1] = off[i] + (0 if sp is None else sp[0].shape[0])
    total = int(off[-1])
    idx = np.zeros(max(total, 1), dtype=np.uint32)
    val = np.zeros(max(total, 1), dtype=np.float32)
    for i, sp in enumerate(sparse_list):
        if sp is not None:
            idx[off[i]:off[i + 1]] = sp[0]
            val[off[i]:off[i + 1]] = sp[1]
    return off, idx, val


def model_term(row_idx, row_val, q_idx, q_val) -> np.float32:
    """The sparse term ``t`` the add kernel gives a row, in numpy float32: from ``+0.0``, over the
    row's entries in ascending index order, ``t = f32(t + f32(v * w))`` for each index the query
    holds too — sequential and unfused, as the kernel's ``__fadd_rn(t, __fmul_rn(v, w))``."""
    row_idx = np.asarray(row_idx, dtype=np.uint32).reshape(-1)
    row_val = np.asarray(row_val, dtype=np.float32).reshape(-1)
    q_idx = np.asarray(q_idx, dtype=np.uint32).reshape(-1)
    q_val = np.asarray(q_val, dtype=np.float32).reshape(-1)
    w = dict(zip(q_idx.tolist(), q_val))
    t = np.float32(0.0)
    with np.errstate(over="ignore"):
        for j in np.argsort(row_idx, kind="stable"):
            qw = w.get(int(row_idx[j]))
            if qw is not None:
                t = np.float32(t + np.float32(row_val[j] * qw))
    return t


def hybrid_convex_scale(dense, sparse, alpha: float):
    """Pinecone's client-side weighting of a hybrid query: ``alpha * dense`` and ``(1 - alpha) *
    sparse`` (``alpha`` in [0, 1]; 1 = dense only).  Returns ``(dense list, sparse dict)``."""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 <= alpha <= 1.0:
        raise ValueError("alpha must be a number in [0, 1]")
    if not isinstance(sparse, dict) or set(sparse) != {"indices", "values"}:
        raise ValueError("sparse must be a dict with exactly the keys 'indices' and 'values'")
    return ([float(v) * alpha for v in dense],
            {"indices": list(sparse["indices"]), "values": [float(v) * (1.0 - alpha) for v in sparse["values"]]})
