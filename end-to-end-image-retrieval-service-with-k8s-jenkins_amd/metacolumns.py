"""Indexed metadata fields as typed device columns, and metadata filters as programs over them.

``Index(..., metadata_config={"indexed": [...]})`` (Pinecone's pod-index knob) keeps the named
fields of every vector's metadata in device memory beside the vectors, so the row-eligibility
bitmap of ``query(filter=...)`` is computed by one kernel (``rc_meta_eval``) instead of a Python
pass over every row (``metafilter.build_bitmap``).  ``metafilter``'s semantics are the
specification: whatever this module cannot express exactly is left to it.

Columns (``Columns``; retrieval_core.h, "Metadata columns"): for F fields over ``capacity`` rows,
``tags`` uint8 [F, capacity] and ``vals`` int64 [F, capacity] on the index's leader device.  One
field of one vector encodes as

    absent                                               tag 0
    type(v) is int with int(float(v)) == v, or float     tag 1, val = the float64 bits
    type(v) is bool                                      tag 2, val = 0 / 1
    type(v) is str                                       tag 3, val = the string's code in the
                                                         field's append-only dictionary

and any other value (a list, a tuple, ``None``, a dict, a subclass of the types above, a numpy
scalar, an int float64 cannot hold) DEMOTES the field: from then on, for the life of the index
object, filters that name it are evaluated on the host.

Programs (``compile_program``): postfix, int64 [n_instr, 2], word 0 = ``op | field << 8 | operand
tag << 16 | k << 32``, word 1 = the operand's val.  Leaves EQ NE GT GE LT LE EXISTS NOT_EXISTS push
one boolean, TRUE / FALSE push a constant, AND(k) / OR(k) fold the top k entries.  ``$in`` is OR
over EQ leaves, ``$nin`` AND over NE leaves, ``$in: []`` FALSE and ``$nin: []`` TRUE; several
operators of a field, or several fields of a dict, are AND.  A string operand the field's
dictionary does not hold gets code -1, which equals nothing.  Children of one AND / OR are ordered
by field (both are commutative), so the kernel loads a field once per run of leaves, and folded two
at a time (``x y AND(2) z AND(2)``), so the stack stays as shallow as the filter's nesting.

Limits: ``MAX_INSTR`` = 512 instructions (a leaf is one, every leaf after the first of its AND / OR
one more: 256 leaves in one ``$in``, more than 64 leaves at any nesting) and a stack of
``MAX_STACK`` = 64 entries (the lane's stack is one 64-bit register; folding holds at most two
entries per level of ``$and`` / ``$or`` — the fields beside it, the list before it — and three at
the innermost field, so 16 levels use at most 35).  Over either,
``compile_program`` returns ``None`` and the host evaluates the filter.

``run_program`` is the numpy model of the kernel: the same program, the same comparison rules, the
same page addressing.  The tests hold the kernel to it and it to ``metafilter``.
"""
from __future__ import annotations

import struct
from typing import Any, Mapping, Sequence

import numpy as np

from . import metafilter

# Rows (or positions of a named namespace) below which a bitmap miss takes the host path even with
# valid columns.  0: measured on an MI355X (tools/metafilter_micro.py, records in
# profiles/metacolumns/metafilter_micro.jsonl, table in DESIGN.md "Metadata columns"), the device
# path's [min, max] lies wholly below the host path's already at 1,000 rows, the smallest size
# measured, for all three filters.
DEVICE_MIN_ROWS = 0

TAG_ABSENT, TAG_NUMBER, TAG_BOOL, TAG_STRING = 0, 1, 2, 3
OP_EQ, OP_NE, OP_GT, OP_GE, OP_LT, OP_LE, OP_EXISTS, OP_NOT_EXISTS, OP_TRUE, OP_FALSE, OP_AND, OP_OR = range(12)
MAX_FIELDS = 64   # RC_META_MAX_FIELDS
MAX_INSTR = 512   # RC_META_MAX_INSTR
MAX_STACK = 64    # RC_META_MAX_STACK

_CMP = {"$gt": OP_GT, "$gte": OP_GE, "$lt": OP_LT, "$lte": OP_LE}


def validate_config(cfg) -> "list[str] | None":
    """The indexed fields of a ``metadata_config`` (``None`` for ``None``); ``ValueError`` unless it is
    a dict with exactly the key ``"indexed"`` holding a list of distinct non-empty strings, none
    starting with ``$``."""
    if cfg is None:
        return None
    if not isinstance(cfg, dict) or set(cfg) != {"indexed"}:
        raise ValueError("metadata_config must be a dict with exactly the key 'indexed'")
    fields = cfg["indexed"]
    if not isinstance(fields, list) or not all(type(f) is str and f for f in fields):
        raise ValueError("metadata_config['indexed'] must be a list of non-empty strings")
    if len(set(fields)) != len(fields):
        raise ValueError("metadata_config['indexed'] names a field twice")
    if any(f.startswith("$") for f in fields):
        raise ValueError("metadata_config['indexed']: a field name cannot start with '$'")
    if len(fields) > MAX_FIELDS:
        raise ValueError(f"metadata_config['indexed'] holds more than {MAX_FIELDS} fields")
    return list(fields)


def float_bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _number_bits(v) -> "int | None":
    """float64 bits of an exact ``int`` / ``float`` (``None`` for an int float64 cannot hold)."""
    if type(v) is float:
        return float_bits(v)
    try:
        f = float(v)
    except OverflowError:
        return None
    return float_bits(f) if int(f) == v else None


def encode_value(v: Any, codes: "dict[str, int]", add: bool = True) -> "tuple[int, int] | None":
    """(tag, val) of a present field value, or ``None`` where the value has no encoding (the field
    demotes; as a filter operand: the host evaluates).  ``codes``: the field's dictionary; ``add``
    gives a new string the next code (upserts), without it an unknown string is code -1
    (operands: it equals nothing)."""
    t = type(v)
    if t is bool:
        return TAG_BOOL, int(v)
    if t is int or t is float:
        b = _number_bits(v)
        return None if b is None else (TAG_NUMBER, b)
    if t is str:
        c = codes.get(v)
        if c is None:
            if not add:
                return TAG_STRING, -1
            c = codes[v] = len(codes)
        return TAG_STRING, c
    return None


class _HostPath(Exception):
    """The filter has no program: the host evaluates it."""


def _leaf(op: int, field: int, tag: int = 0, val: int = 0):
    return ("leaf", op, field, tag, val)


def _fold(kind: str, children: list):
    if len(children) == 1:
        return children[0]
    # leaves first, by field (stable): one column load per run of leaves on a field
    return (kind, sorted(children, key=lambda c: (0, c[2]) if c[0] == "leaf" else (1, 0)))


def _tree(flt: Mapping[str, Any], index: Mapping[str, int], dictionaries: Mapping[str, dict]):
    out = []
    for key, val in flt.items():
        if key in ("$and", "$or"):
            out.append(_fold("and" if key == "$and" else "or", [_tree(x, index, dictionaries) for x in val]))
            continue
        f = index.get(key)
        if f is None:
            raise _HostPath(key)
        codes = dictionaries[key]

        def operand(o):
            e = encode_value(o, codes, add=False)
            if e is None:
                raise _HostPath(key)
            return e

        for op, o in (val.items() if isinstance(val, Mapping) else (("$eq", val),)):
            if op == "$eq":
                out.append(_leaf(OP_EQ, f, *operand(o)))
            elif op == "$ne":
                out.append(_leaf(OP_NE, f, *operand(o)))
            elif op == "$in":
                out.append(_fold("or", [_leaf(OP_EQ, f, *operand(x)) for x in o]) if len(o) else ("const", False))
            elif op == "$nin":
                out.append(_fold("and", [_leaf(OP_NE, f, *operand(x)) for x in o]) if len(o) else ("const", True))
            elif op in _CMP:
                out.append(_leaf(_CMP[op], f, *operand(o)))
            else:  # "$exists" (compile_filter refused every other operator)
                out.append(_leaf(OP_EXISTS if o else OP_NOT_EXISTS, f))
    if not out:
        return ("const", True)
    return _fold("and", out)


def _emit(node, out: list) -> None:
    if node[0] == "leaf":
        _, op, f, tag, val = node
        out.append((op | f << 8 | tag << 16, val))
    elif node[0] == "const":
        out.append((OP_TRUE if node[1] else OP_FALSE, 0))
    else:
        word = (OP_AND if node[0] == "and" else OP_OR) | 2 << 32
        _emit(node[1][0], out)
        for c in node[1][1:]:
            _emit(c, out)
            out.append((word, 0))


def check_program(program, n_fields: int) -> None:
    """``ValueError`` unless the program is one ``rc_meta_eval`` accepts (the same checks)."""
    prog = np.asarray(program)
    if prog.dtype != np.int64 or prog.ndim != 2 or prog.shape[1] != 2 or not 1 <= prog.shape[0] <= MAX_INSTR:
        raise ValueError(f"a program is int64 [n_instr, 2] with 1 <= n_instr <= {MAX_INSTR}")
    depth = 0
    for w0 in prog[:, 0].tolist():
        op, f, tag, k = w0 & 0xFF, (w0 >> 8) & 0xFF, (w0 >> 16) & 0xFF, w0 >> 32
        if w0 < 0 or (w0 >> 24) & 0xFF:
            raise ValueError("malformed program word")
        if op <= OP_NOT_EXISTS:
            if f >= n_fields:
                raise ValueError("program names a field at or past n_fields")
            if op <= OP_LE and not TAG_NUMBER <= tag <= TAG_STRING:
                raise ValueError("bad operand tag")
            depth += 1
        elif op in (OP_TRUE, OP_FALSE):
            depth += 1
        elif op in (OP_AND, OP_OR):
            if not 1 <= k <= depth:
                raise ValueError("program underflows its stack")
            depth -= k - 1
        else:
            raise ValueError("unknown program op")
        if depth > MAX_STACK:
            raise ValueError("program passes MAX_STACK")
    if depth != 1:
        raise ValueError("program must leave exactly one result")


def compile_program(flt: Mapping[str, Any], fields: Sequence[str], dictionaries: Mapping[str, dict],
                    demoted=()) -> "np.ndarray | None":
    """The program of a metadata filter over the columns of ``fields`` (column f holds
    ``fields[f]``), int64 [n_instr, 2], or ``None`` where the host must evaluate it: the filter
    names a field that is not in ``fields`` or is in ``demoted``, an operand is not exactly a
    ``bool`` / ``int`` / ``float`` / ``str`` (or is an int float64 cannot hold), or the program
    passes ``MAX_INSTR`` or ``MAX_STACK``.  A malformed filter raises what
    ``metafilter.compile_filter`` raises.  ``dictionaries``: field -> {string: code}; read only."""
    metafilter.compile_filter(flt)
    index = {name: f for f, name in enumerate(fields) if name not in demoted}
    try:
        tree = _tree(flt, index, dictionaries)
    except _HostPath:
        return None
    out: list = []
    _emit(tree, out)
    if len(out) > MAX_INSTR:
        return None
    prog = np.array(out, dtype=np.int64).reshape(-1, 2)
    try:
        check_program(prog, len(fields))
    except ValueError:  # deeper than MAX_STACK
        return None
    return prog


def run_program(program, tags, vals, n: int, pages=None, span: int = 0) -> "tuple[np.ndarray, int]":
    """What ``rc_meta_eval`` computes, in numpy: (bitmap uint32 [ceil(n / 32)], eligible count) of
    the program over positions [0, n) of the columns ``tags`` uint8 [F, capacity] / ``vals`` int64
    [F, capacity].  Position p is row p, or with a page list row ``pages[p // span] * span + p % span``."""
    tags = np.asarray(tags, dtype=np.uint8)
    vals = np.asarray(vals, dtype=np.int64)
    prog = np.asarray(program, dtype=np.int64)
    check_program(prog, tags.shape[0])
    n = int(n)
    pos = np.arange(n, dtype=np.int64)
    if pages is None:
        rows = pos
    else:
        pg = np.asarray(pages, dtype=np.int64).reshape(-1)
        if span < 256 or span % 256 or n > pg.shape[0] * span:
            raise ValueError("span must be a positive multiple of 256 and n inside the page list")
        rows = pg[pos // span] * span + pos % span
    if n and (rows.min() < 0 or rows.max() >= tags.shape[1]):
        raise ValueError("a position outside the columns")
    stack: list[np.ndarray] = []
    for w0, ov in prog.tolist():
        op, f, ot, k = w0 & 0xFF, (w0 >> 8) & 0xFF, (w0 >> 16) & 0xFF, w0 >> 32
        if op <= OP_NOT_EXISTS:
            t, v = tags[f, rows], vals[f, rows]
            a, b = v.view(np.float64), np.array(ov, dtype=np.int64).view(np.float64)
            with np.errstate(invalid="ignore"):
                num = (t == TAG_NUMBER) & (ot == TAG_NUMBER)
                eq = (t == ot) & np.where(t == TAG_NUMBER, a == b, v == ov)
                r = {OP_EQ: lambda: eq, OP_NE: lambda: ~eq, OP_GT: lambda: num & (a > b), OP_GE: lambda: num & (a >= b),
                     OP_LT: lambda: num & (a < b), OP_LE: lambda: num & (a <= b), OP_EXISTS: lambda: t != TAG_ABSENT,
                     OP_NOT_EXISTS: lambda: t == TAG_ABSENT}[op]()
            stack.append(np.asarray(r, dtype=bool))
        elif op in (OP_TRUE, OP_FALSE):
            stack.append(np.full(n, op == OP_TRUE, dtype=bool))
        else:
            top, stack = stack[-k:], stack[:-k]
            stack.append(np.logical_and.reduce(top) if op == OP_AND else np.logical_or.reduce(top))
    flags = stack[0]
    return metafilter.pack_bits(flags), int(flags.sum())


class FieldIndex:
    """Host state of an index's metadata columns, shared by its column sets (the default
    namespace's and the pool's): the configured fields, one append-only string dictionary per
    field, the demoted fields, whether the device columns can be trusted, and the counters of
    ``Index.metadata_index_stats``."""

    def __init__(self, fields: Sequence[str]):
        self.fields = list(fields)
        self.dictionaries: dict[str, dict[str, int]] = {f: {} for f in self.fields}
        self.demoted: dict[str, str] = {}
        self.valid = True
        self.device_evals = 0
        self.host_evals = 0

    def encode(self, metas: Sequence[Mapping[str, Any]]) -> "tuple[np.ndarray, np.ndarray]":
        """(tags uint8 [F, m], vals int64 [F, m]) of m metadata dicts.  A value without an encoding
        demotes its field (its column is no longer read; the rest of the batch encodes on)."""
        m = len(metas)
        tags = np.zeros((len(self.fields), m), dtype=np.uint8)
        vals = np.zeros((len(self.fields), m), dtype=np.int64)
        for f, name in enumerate(self.fields):
            if name in self.demoted:
                continue
            codes = self.dictionaries[name]
            for i, md in enumerate(metas):
                if name not in md:
                    continue
                e = encode_value(md[name], codes)
                if e is None:
                    self.demoted[name] = f"a value of type {type(md[name]).__name__} has no column encoding"
                    tags[f], vals[f] = 0, 0
                    break
                tags[f, i], vals[f, i] = e
        return tags, vals

    def program(self, flt) -> "np.ndarray | None":
        return compile_program(flt, self.fields, self.dictionaries, self.demoted)

    def stats(self) -> dict:
        return {"indexed": list(self.fields), "device": [f for f in self.fields if f not in self.demoted],
                "demoted": dict(self.demoted), "valid": self.valid, "device_evals": self.device_evals,
                "host_evals": self.host_evals}


class Columns:
    """One column set on one device: ``tags`` uint8 [F, capacity], ``vals`` int64 [F, capacity]
    (torch tensors), written, moved and evaluated by the library's ``rc_meta_*`` entries on the
    device's current stream."""

    def __init__(self, n_fields: int, capacity: int, device):
        import torch

        from . import _lib

        self._torch, self._lib = torch, _lib
        self.lib = _lib.load()
        self.n_fields = int(n_fields)
        self.device = torch.device(device)
        self.capacity = max(1, int(capacity))
        self.tags = torch.zeros((self.n_fields, self.capacity), dtype=torch.uint8, device=self.device)
        self.vals = torch.zeros((self.n_fields, self.capacity), dtype=torch.int64, device=self.device)

    def ensure(self, capacity: int) -> None:
        """Grow to at least ``capacity`` rows (the owner doubles its vectors' capacity; the
        columns follow it), keeping what is stored."""
        capacity = int(capacity)
        if capacity <= self.capacity:
            return
        torch = self._torch
        tags = torch.zeros((self.n_fields, capacity), dtype=torch.uint8, device=self.device)
        vals = torch.zeros((self.n_fields, capacity), dtype=torch.int64, device=self.device)
        tags[:, :self.capacity] = self.tags
        vals[:, :self.capacity] = self.vals
        self.tags, self.vals, self.capacity = tags, vals, capacity

    def _rows(self, rows):
        torch = self._torch
        r = torch.as_tensor(rows, dtype=torch.int64).reshape(-1)
        if r.numel() and (int(r.min()) < 0 or int(r.max()) >= self.capacity):
            raise ValueError("a row outside the metadata columns")
        return r.to(self.device).contiguous()

    def write(self, rows, tags: np.ndarray, vals: np.ndarray) -> None:
        """All F fields of the distinct rows ``rows``: ``tags`` / ``vals`` [F, len(rows)] (rc_meta_write)."""
        torch, L = self._torch, self._lib
        if tags.shape != (self.n_fields, len(rows)) or vals.shape != tags.shape:
            raise ValueError("tags and vals must be [n_fields, len(rows)]")
        with torch.cuda.device(self.device):
            r = self._rows(rows)
            t = torch.from_numpy(np.ascontiguousarray(tags, dtype=np.uint8)).to(self.device)
            v = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.int64)).to(self.device)
            L.check(self.lib.rc_meta_write(L.ptr(self.tags), L.ptr(self.vals), self.n_fields, self.capacity, L.ptr(r),
                                           L.ptr(t), L.ptr(v), r.numel(), L.stream_ptr()))
            torch.cuda.current_stream().synchronize()

    def move(self, src, dst) -> None:
        """Row dst[i] becomes a copy of row src[i] in every field (rc_meta_move; disjoint lists)."""
        torch, L = self._torch, self._lib
        if len(src) != len(dst):
            raise ValueError("src and dst differ in length")
        with torch.cuda.device(self.device):
            s, d = self._rows(src), self._rows(dst)
            L.check(self.lib.rc_meta_move(L.ptr(self.tags), L.ptr(self.vals), self.n_fields, self.capacity, L.ptr(s),
                                          L.ptr(d), s.numel(), L.stream_ptr()))
            torch.cuda.current_stream().synchronize()

    def eval(self, program: np.ndarray, n: int, pages=None, span: int = 0) -> "tuple[np.ndarray, int]":
        """(bitmap uint32 [ceil(n / 32)], eligible count) of ``program`` over positions [0, n)
        (rc_meta_eval): what ``run_program`` returns, one kernel and one synchronisation."""
        torch, L = self._torch, self._lib
        prog = np.ascontiguousarray(program, dtype=np.int64)
        n = int(n)
        words = (n + 31) // 32
        pg = None if pages is None else np.ascontiguousarray(pages, dtype=np.int32).reshape(-1)
        n_pages = 0 if pg is None else int(pg.shape[0])
        with torch.cuda.device(self.device):
            ws = torch.empty((16 * prog.shape[0] + 4 * n_pages,), dtype=torch.uint8, device=self.device)
            out = torch.empty((words + 1,), dtype=torch.int32, device=self.device)  # the words, then the count
            L.check(self.lib.rc_meta_eval(L.ptr(self.tags), L.ptr(self.vals), self.n_fields, self.capacity,
                                          prog.ctypes.data, prog.shape[0], None if pg is None else pg.ctypes.data, n_pages,
                                          int(span), n, L.ptr(ws), ws.numel(), L.ptr(out), L.ptr(out) + 4 * words,
                                          L.stream_ptr()))
            host = out.cpu().numpy().view(np.uint32)  # the one synchronisation; prog and pg are alive until here
        return host[:words].copy(), int(host[words])
