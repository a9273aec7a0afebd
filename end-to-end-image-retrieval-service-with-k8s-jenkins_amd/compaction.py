"""Swap-remove compaction plan of ``Index.delete`` (pure Python: no torch, no device).

The index keeps its live rows dense: an id's row is its position in ``Index._ids`` and every
search takes ``n_rows``.  Deleting the rows ``D`` of ``n`` leaves ``n' = n - |D|`` rows; each
hole (a deleted row below ``n'``) is filled with one surviving row of the tail ``[n', n)``, and
the length drops to ``n'``.  There are exactly as many holes as tail survivors (both are ``|D|``
minus the deleted rows of the tail), so the plan is a pairing of the two sets, and the only
device work is moving at most ``|D|`` stored rows.

Global row ``g`` lives on shard ``g % n_shards``.  A hole is paired with a survivor of its own
shard wherever one exists (that move stays inside one GPU); what is left over is paired in
ascending order and crosses shards.  The number of same-shard pairs, the sum over the shards of
min(holes, survivors), is the most any pairing can have.

The cost is O(|D| log |D|): the tail has |D| rows, so nothing here walks the ``n`` rows.
"""
from __future__ import annotations

from typing import Iterable


def plan_compaction(n: int, deleted_rows: Iterable[int], n_shards: int = 1) -> tuple[list[int], list[int]]:
    """``(src, dst)``: stored row ``dst[i]`` takes the content of row ``src[i]``, then the first
    ``n - |deleted_rows|`` rows are the survivors, each exactly once.  ``dst`` is the holes in
    ascending order, ``src`` a permutation of the tail survivors; the two are disjoint.  Repeated
    entries of ``deleted_rows`` count once; a row outside ``[0, n)`` is a ``ValueError``."""
    n, n_shards = int(n), int(n_shards)
    if n < 0 or n_shards < 1:
        raise ValueError("n must be >= 0 and n_shards >= 1")
    dead = sorted({int(r) for r in deleted_rows})
    if dead and (dead[0] < 0 or dead[-1] >= n):
        raise ValueError("deleted row out of range")
    new_n = n - len(dead)
    holes = [r for r in dead if r < new_n]
    dead_tail = set(dead[len(holes):])
    survivors = [r for r in range(new_n, n) if r not in dead_tail]
    if n_shards == 1:
        return survivors, holes
    by_shard: dict[int, list[int]] = {}
    for r in reversed(survivors):  # popped from the end: ascending
        by_shard.setdefault(r % n_shards, []).append(r)
    fill: dict[int, int] = {}
    rest_holes = []
    for hole in holes:
        own = by_shard.get(hole % n_shards)
        if own:
            fill[hole] = own.pop()
        else:
            rest_holes.append(hole)
    rest = sorted(r for own in by_shard.values() for r in own)
    fill.update(zip(rest_holes, rest))
    return [fill[hole] for hole in holes], holes
