"""Seeded metadata dicts and metadata filters for the metadata-column tests (CPU and GPU).

Five fields, each holding strings, numbers and booleans in different rows (so every typed
comparison meets every tag), about 30 % of the fields absent.  The filters nest to depth 3, use
every operator of ``metafilter`` — empty ``$in`` / ``$nin`` and strings no row holds included — and
only operands with a column encoding, so each of them must compile to a program."""
import random

import numpy as np

FIELDS = ["color", "size", "flag", "score", "tag"]
STRINGS = ["red", "green", "blue", "", "Red"]
NUMBERS = [0, 1, -1, 3, 7, 2.5, 1.0, -0.0, 0.0, -3.25, 1e300, 2 ** 53]
SPECIAL = [float("nan"), float("inf"), float("-inf")]
UNKNOWN = ["no-row-holds-this", "nor-this"]
OPS = ["$eq", "$ne", "$gt", "$gte", "$lt", "$lte", "$in", "$nin", "$exists"]


def _value(rng, special):
    r = rng.random()
    if r < 0.4:
        return rng.choice(STRINGS)
    if r < 0.85:
        return rng.choice(NUMBERS + (SPECIAL if special else []))
    return rng.random() < 0.5


def gen_metas(n, seed, special=True):
    """n metadata dicts; ``special`` adds NaN and the infinities to the numbers."""
    rng = random.Random(seed)
    return [{f: _value(rng, special) for f in FIELDS if rng.random() >= 0.3} for _ in range(n)]


def _operand(rng, special):
    if rng.random() < 0.15:
        return rng.choice(UNKNOWN)
    return _value(rng, special)


def _cond(rng, special):
    if rng.random() < 0.2:
        return _operand(rng, special)  # a bare value: $eq
    out = {}
    for op in rng.sample(OPS, rng.choice([1, 1, 2])):
        if op in ("$eq", "$ne"):
            out[op] = _operand(rng, special)
        elif op in ("$in", "$nin"):
            out[op] = [_operand(rng, special) for _ in range(rng.choice([0, 1, 2, 3, 5]))]
        elif op == "$exists":
            out[op] = rng.random() < 0.5
        else:
            out[op] = rng.choice(NUMBERS + (SPECIAL if special else []))
    return out


def _filter(rng, depth, special):
    if depth > 0 and rng.random() < 0.4:
        return {rng.choice(["$and", "$or"]): [_filter(rng, depth - 1, special) for _ in range(rng.choice([1, 2, 3]))]}
    out = {f: _cond(rng, special) for f in rng.sample(FIELDS, rng.choice([1, 1, 2]))}
    if depth > 0 and rng.random() < 0.25:
        out[rng.choice(["$and", "$or"])] = [_filter(rng, depth - 1, special) for _ in range(rng.choice([1, 2]))]
    return out


def gen_filters(count, seed, special=True):
    """count filters nested to depth 3.  ``special=False`` keeps NaN and the infinities out of the
    operands (``Index`` refuses filters that are not strict JSON)."""
    rng = random.Random(seed)
    return [_filter(rng, 3, special) for _ in range(count)]


def ops_used(flt, acc=None):
    acc = set() if acc is None else acc
    for k, v in flt.items():
        if k in ("$and", "$or"):
            acc.add(k)
            for x in v:
                ops_used(x, acc)
        elif isinstance(v, dict):
            acc.update(v)
        else:
            acc.add("bare")
    return acc


def depth_of(flt):
    return 1 + max([depth_of(x) for k, v in flt.items() if k in ("$and", "$or") for x in v], default=0)


def encode_all(mc, metas, fields=FIELDS, capacity=None, decoys=None):
    """(FieldIndex, tags [F, capacity], vals [F, capacity]): ``metas`` encoded into rows
    [0, len(metas)), and ``decoys`` (metadata dicts) repeated over the rows past them."""
    fx = mc.FieldIndex(fields)
    n = len(metas)
    capacity = n if capacity is None else capacity
    rest = [decoys[i % len(decoys)] for i in range(capacity - n)] if decoys else [{}] * (capacity - n)
    tags, vals = fx.encode(list(metas) + rest)
    assert fx.demoted == {}
    return fx, np.ascontiguousarray(tags), np.ascontiguousarray(vals)
