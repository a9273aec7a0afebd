"""Pinecone-style metadata filters: ``index.query(..., filter={...})``.

Pure Python, no GPU use.  ``compile_filter`` turns a filter dict into a predicate over one
vector's metadata dict; ``build_bitmap`` evaluates the predicate over the index's rows and packs
the answers into the row-eligibility bitmap the masked search takes
(``rc_sharded_search_masked``: little-endian ``uint32`` words, bit ``r & 31`` of word ``r >> 5``
= row ``r`` is eligible, ``ceil(n_rows / 32)`` words, padding bits clear).

The language
  field operators  ``$eq $ne $gt $gte $lt $lte $in $nin $exists``
  logical          ``$and`` / ``$or`` (a list of filter dicts)
  several fields (or operators of one field) in one dict mean AND; a bare value means ``$eq``.

Pinecone's server is closed, so the semantics are fixed here (INTEGRATION.md repeats them):
  * a comparison on a missing field is false, except ``$ne`` and ``$nin``, which are true;
  * ``$gt $gte $lt $lte`` compare numbers with numbers only (``bool`` is not a number): any
    other pairing is false;
  * equality is typed the same way: ``True`` does not equal ``1``, ``1`` equals ``1.0``;
  * a list-valued field matches ``$eq`` / ``$in`` if any element does (``$ne`` / ``$nin`` are
    their negations);
  * ``$exists: true`` holds when the field is present, ``$exists: false`` when it is not;
  * an unknown operator or a malformed operand (``$in`` without a list, ``$and`` without a
    list of dicts, ``$gt`` with a non-number, ``$exists`` with a non-bool, a field name
    starting with ``$``) raises ``ValueError``.
"""
from __future__ import annotations

import json
from typing import Any, Callable, Iterable, Mapping, Sequence

import numpy as np

Predicate = Callable[[Mapping[str, Any]], bool]

_MISSING = object()


def _is_number(v: Any) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _scalar_eq(a: Any, b: Any) -> bool:
    if isinstance(a, bool) or isinstance(b, bool):
        return isinstance(a, bool) and isinstance(b, bool) and a == b
    if _is_number(a) and _is_number(b):
        return a == b
    return type(a) is type(b) and a == b


def _field_eq(field: Any, operand: Any) -> bool:
    if isinstance(field, (list, tuple)):
        return any(_scalar_eq(e, operand) for e in field)
    return _scalar_eq(field, operand)


def _check_scalar(op: str, v: Any) -> None:
    if not (isinstance(v, (str, bool)) or _is_number(v)):
        raise ValueError(f"{op} needs a string, number or boolean operand (got {type(v).__name__})")


def _compile_op(field: str, op: str, operand: Any) -> Predicate:
    if op == "$eq":
        _check_scalar(op, operand)
        return lambda md: (v := md.get(field, _MISSING)) is not _MISSING and _field_eq(v, operand)
    if op == "$ne":
        _check_scalar(op, operand)
        return lambda md: (v := md.get(field, _MISSING)) is _MISSING or not _field_eq(v, operand)
    if op in ("$in", "$nin"):
        if not isinstance(operand, (list, tuple)):
            raise ValueError(f"{op} needs a list operand")
        for o in operand:
            _check_scalar(op, o)
        ops = list(operand)
        if op == "$in":
            return lambda md: (v := md.get(field, _MISSING)) is not _MISSING and any(_field_eq(v, o) for o in ops)
        return lambda md: (v := md.get(field, _MISSING)) is _MISSING or not any(_field_eq(v, o) for o in ops)
    if op in ("$gt", "$gte", "$lt", "$lte"):
        if not _is_number(operand):
            raise ValueError(f"{op} needs a number operand (got {type(operand).__name__})")
        cmp = {"$gt": lambda a: a > operand, "$gte": lambda a: a >= operand, "$lt": lambda a: a < operand,
               "$lte": lambda a: a <= operand}[op]
        return lambda md: _is_number(v := md.get(field, _MISSING)) and cmp(v)
    if op == "$exists":
        if not isinstance(operand, bool):
            raise ValueError("$exists needs a boolean operand")
        return lambda md: (field in md) == operand
    raise ValueError(f"unknown filter operator {op!r}")


def _all(preds: Sequence[Predicate]) -> Predicate:
    if len(preds) == 1:
        return preds[0]
    return lambda md: all(p(md) for p in preds)


def compile_filter(flt: Mapping[str, Any]) -> Predicate:
    """The predicate of a filter dict (``ValueError`` if it is malformed).  ``{}`` matches all."""
    if not isinstance(flt, Mapping):
        raise ValueError("a filter must be a dict")
    preds: list[Predicate] = []
    for key, val in flt.items():
        if not isinstance(key, str):
            raise ValueError("filter keys must be strings")
        if key in ("$and", "$or"):
            if not isinstance(val, (list, tuple)) or not val or not all(isinstance(x, Mapping) for x in val):
                raise ValueError(f"{key} needs a non-empty list of filter dicts")
            subs = [compile_filter(x) for x in val]
            preds.append(_all(subs) if key == "$and" else (lambda md, subs=subs: any(p(md) for p in subs)))
        elif key.startswith("$"):
            raise ValueError(f"unknown filter operator {key!r}")
        elif isinstance(val, Mapping):
            if not val:
                raise ValueError(f"field {key!r} has an empty operator dict")
            preds.extend(_compile_op(key, op, operand) for op, operand in val.items())
        else:
            preds.append(_compile_op(key, "$eq", val))
    if not preds:
        return lambda md: True
    return _all(preds)


def canonical(flt: Mapping[str, Any]) -> str:
    """A filter's canonical JSON (sorted keys): equal filters share one cache entry."""
    try:
        return json.dumps(flt, sort_keys=True, separators=(",", ":"), allow_nan=False)
    except (TypeError, ValueError) as e:
        raise ValueError(f"a filter must be JSON-serialisable: {e}") from None


def pack_bits(flags: "np.ndarray | Iterable[bool]") -> np.ndarray:
    """bool [n] → little-endian uint32 [ceil(n / 32)]: bit r & 31 of word r >> 5 = flags[r]."""
    f = np.asarray(flags, dtype=bool).reshape(-1)
    n = f.shape[0]
    words = (n + 31) // 32
    padded = np.zeros(words * 32, dtype=bool)
    padded[:n] = f
    by = np.packbits(padded, bitorder="little")  # byte b holds rows 8b .. 8b + 7, lowest bit first
    return by.view(np.dtype("<u4")).astype(np.uint32, copy=False)


def build_bitmap(pred: Predicate, ids: Sequence[str], meta: Mapping[str, Mapping[str, Any]]) -> tuple[np.ndarray, int]:
    """(bitmap, eligible count) over the rows of ``ids`` (row r holds ``ids[r]``; a vector
    without metadata has ``{}``)."""
    empty: dict = {}
    flags = np.fromiter((bool(pred(meta.get(i, empty))) for i in ids), dtype=bool, count=len(ids))
    return pack_bits(flags), int(flags.sum())
