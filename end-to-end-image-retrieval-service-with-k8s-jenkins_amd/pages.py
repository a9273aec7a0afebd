"""Page bookkeeping of the index's named namespaces (pure Python: no torch, no device).

Every named namespace lives in one second ``ShardSet``, the pool.  The pool's rows are handed
out in pages of ``PAGE_ROWS`` local rows per shard: with ``S`` shards, page ``p`` is local rows
``[PAGE_ROWS p, PAGE_ROWS (p + 1))`` on EVERY shard, i.e. pool rows ``[span p, span (p + 1))``
with ``span = PAGE_ROWS S``.  A namespace is an ordered page list ``L`` and a count ``n``; its
vectors are dense in position space ``[0, n)``, position ``i`` at pool row
``L[i // span] * span + i % span``.  A pool row ``g`` is on shard ``g % S``; ``span`` is a multiple
of ``S``, so position ``i`` is on shard ``i % S`` too — a namespace is spread over the shards
exactly as a dense index of its own would be, which is what lets the delete planner
(``compaction.plan_compaction``) and the searches' cross-shard merge work on positions unchanged.

``PageAllocator`` hands pages out: freed pages first (lowest number first), then fresh ones
past the high-water mark; ``pages_needed`` beyond what the pool holds is the caller's signal to
grow the pool (``capacity_needed``) before it writes.
"""
from __future__ import annotations

from typing import Iterable, Sequence

PAGE_ROWS = 256  # local rows per shard in one page (RC_PAGE_ROWS in retrieval_core.h)


def span(n_shards: int) -> int:
    """Pool rows (= positions) one page covers over ``n_shards`` shards."""
    n_shards = int(n_shards)
    if n_shards < 1:
        raise ValueError("n_shards must be >= 1")
    return PAGE_ROWS * n_shards


def pages_for(n: int, n_shards: int) -> int:
    """Pages a namespace of ``n`` vectors holds: ``ceil(n / (PAGE_ROWS S))``."""
    n = int(n)
    if n < 0:
        raise ValueError("n must be >= 0")
    return -(-n // span(n_shards))


def position_to_row(page_list: Sequence[int], position: int, n_shards: int) -> int:
    """Pool row of a namespace position."""
    sp = span(n_shards)
    position = int(position)
    if position < 0 or position >= len(page_list) * sp:
        raise ValueError("position outside the namespace's pages")
    return int(page_list[position // sp]) * sp + position % sp


def positions_to_rows(page_list: Sequence[int], positions: Iterable[int], n_shards: int) -> list[int]:
    return [position_to_row(page_list, p, n_shards) for p in positions]


def row_to_position(page_list: Sequence[int], row: int, n_shards: int) -> int:
    """Inverse of ``position_to_row`` (``ValueError`` for a row of a page the list does not hold)."""
    sp = span(n_shards)
    row = int(row)
    page = row // sp
    for e, p in enumerate(page_list):
        if p == page:
            return e * sp + row % sp
    raise ValueError("row is in none of the namespace's pages")


def row_runs(page_list: Sequence[int], n: int, n_shards: int) -> list[tuple[int, int, int]]:
    """The positions ``[0, n)`` as runs ``(position0, pool_row0, count)`` of consecutive pool rows,
    runs of consecutive pages coalesced: what an export or import of the namespace copies."""
    sp = span(n_shards)
    runs: list[tuple[int, int, int]] = []
    for e in range(pages_for(n, n_shards)):
        pos0 = e * sp
        cnt = min(sp, n - pos0)
        row0 = int(page_list[e]) * sp
        if runs and runs[-1][1] + runs[-1][2] == row0 and runs[-1][0] + runs[-1][2] == pos0:
            runs[-1] = (runs[-1][0], runs[-1][1], runs[-1][2] + cnt)
        else:
            runs.append((pos0, row0, cnt))
    return runs


class PageAllocator:
    """Free list plus a high-water mark over the pool's pages.

    ``capacity_pages`` is how many pages the pool's current capacity holds
    (``capacity_per_shard // PAGE_ROWS``); ``alloc`` never hands out a page at or past it —
    the caller grows the pool first (``pages_short`` / ``capacity_needed``) and reports the new
    size with ``set_capacity``.  The pool never shrinks."""

    def __init__(self, capacity_pages: int = 0):
        self.capacity_pages = int(capacity_pages)
        self.high_water = 0          # pages [0, high_water) were handed out at least once
        self._free: list[int] = []   # kept sorted descending: pop() gives the lowest page

    @property
    def free_pages(self) -> int:
        return len(self._free) + self.capacity_pages - self.high_water

    @property
    def used_pages(self) -> int:
        return self.high_water - len(self._free)

    def set_capacity(self, capacity_pages: int) -> None:
        capacity_pages = int(capacity_pages)
        if capacity_pages < self.capacity_pages:
            raise ValueError("the pool never shrinks")
        self.capacity_pages = capacity_pages

    def pages_short(self, count: int) -> int:
        """How many of ``count`` pages the pool cannot hand out at its current capacity."""
        return max(0, int(count) - self.free_pages)

    def capacity_needed(self, count: int, per_shard: int) -> int:
        """The capacity per shard (``per_shard`` doubled until it fits, a whole number of pages)
        at which ``count`` more pages can be handed out; ``per_shard`` if they already can."""
        need = (self.used_pages + int(count)) * PAGE_ROWS
        per = max(int(per_shard), PAGE_ROWS)
        while per < need:
            per *= 2
        return -(-per // PAGE_ROWS) * PAGE_ROWS

    def alloc(self, count: int = 1) -> list[int]:
        count = int(count)
        if count < 0:
            raise ValueError("count must be >= 0")
        if self.pages_short(count):
            raise MemoryError("the pool has no free page: grow it first (capacity_needed)")
        out = []
        for _ in range(count):
            if self._free:
                out.append(self._free.pop())
            else:
                out.append(self.high_water)
                self.high_water += 1
        return out

    def free(self, page_list: Iterable[int]) -> None:
        got = [int(p) for p in page_list]
        held = set(self._free)
        for p in got:
            if p < 0 or p >= self.high_water or p in held:
                raise ValueError(f"page {p} is not allocated")
            held.add(p)
        self._free = sorted(held, reverse=True)
