"""Staging `.kin[.bgz]` tables in HBM: the one budget rule, the one cut rule and the one upload loop of the merger, the query
and the extract paths.

A pass over addresses [lo, hi) of N tables asks hbm_budget for the bytes it may fill, sub_slices for the cuts at which N
slices fit that budget beside each other, and staged_pieces for the pieces themselves: every cut of every table read (or
inflated) from its file and uploaded, one piece after the other -- a piece is uploaded, then scanned, then the next one is
uploaded.  Tables that lie in HBM already (ResidentTable) are scanned where they are.
"""
import os
from concurrent.futures import ThreadPoolExecutor

from . import _lib, bgzf


def hbm_budget(device: int, budget: int = None, workspace: int = 0) -> int:
    """The bytes of HBM a pass may fill with staged slices and what it keeps beside them: `budget` if given, else
    PK_MERGE_HBM_BUDGET, else 80 % of the free HBM less `workspace` bytes (what the pass needs besides and does not budget
    itself; neither a given budget nor the environment's is reduced by it)."""
    return int(budget or 0) or int(os.environ.get("PK_MERGE_HBM_BUDGET", "0")) or \
        max(0, int(_lib.mem_info(device)[0] * 0.8) - workspace)


def sub_slices(lo: int, hi: int, n_tables: int, device: int, reserve: int = 0, budget: int = None):
    """[lo, hi) cut so that n_tables slices fit HBM beside each other (the reference streams pairs and takes
    any N, merger.py:139-153; here a k=17 merge of 32 tables is 512 GiB).  Partials add, so the cuts are free.
    The budget is hbm_budget's; `reserve` bytes of it are kept for something else (a spectrum accumulator: 41 MB at
    N = 13, 4.2 GB at N = 128)."""
    budget = hbm_budget(device, budget)
    budget -= reserve
    per_table = max(2048, (budget // max(1, n_tables) - 64) & ~2047)
    return [(a, min(hi, a + per_table)) for a in range(lo, hi, per_table)]


class ResidentTable:
    """Addresses [first, first + n) of one 4^k-byte table that already lie in HBM on `device` (e.g. the table of an
    indexer that has just finished: pk_indexer_table_device) -- takes a Header's place in pair_matrix / gpu_partial, which
    then scan it where it is instead of staging it from a file."""

    def __init__(self, ptr: int, n: int, data_size: int, device: int = 0, first: int = 0):
        assert ptr % 16 == 0 and first % 32 == 0
        self.ptr, self.n, self.data_size, self.device, self.first = int(ptr), int(n), int(data_size), device, int(first)

    def device_slice(self, lo: int, hi: int) -> int:
        assert self.first <= lo <= hi <= self.first + self.n, "address range outside the resident part of the table"
        return self.ptr + (lo - self.first)


def all_resident(tables) -> bool:
    """Whether the tables lie in HBM already (they all do or none does: a pass stages either everything or nothing)."""
    resident = [hasattr(t, "device_slice") for t in tables]
    assert all(resident) or not any(resident), "resident and file-backed tables cannot be mixed in one pass"
    return all(resident)


def piece_cuts(tables, lo: int, hi: int, staged_tables: int, device: int, reserve: int = 0, budget: int = None):
    """The cuts of a pass over [lo, hi): sub_slices' for `staged_tables` slices beside each other, or the one piece [lo, hi)
    of tables that are resident, for which nothing has to fit (and the free HBM is not asked for)."""
    return [(lo, hi)] if all_resident(tables) else sub_slices(lo, hi, staged_tables, device, reserve=reserve, budget=budget)


def staged_pieces(tables, cuts, device: int, threads: int):
    """Yields (ptrs, a, b) for every [a, b) of `cuts`, in their order: the device pointers of addresses [a, b) of every
    table.  File-backed tables (anything with read_table_slice(lo, hi, threads=)) are staged in one DeviceBuffer each, as
    large as the largest cut and filled again for every piece: `threads` tables are read / inflated at a time, each
    .kin.bgz on its share of the native inflate threads, and uploaded as each one lands.  The pointers of a piece hold
    until the next one is asked for; the buffers are freed when the generator is exhausted or closed, or when a read, an
    upload or the consumer raises.  ResidentTables are yielded where they lie, with nothing allocated."""
    if all_resident(tables):
        for a, b in cuts:
            yield [t.device_slice(a, b) for t in tables], a, b
        return
    N = len(tables)
    io_threads = max(1, bgzf.INFLATE_THREADS // max(1, min(threads, N)))
    bufs = []
    try:
        for _ in range(N):
            bufs.append(_lib.DeviceBuffer(max(b - a for a, b in cuts), device))
        with ThreadPoolExecutor(max_workers=max(1, threads)) as pool:
            for a, b in cuts:
                list(pool.map(lambda i: bufs[i].upload(tables[i].read_table_slice(a, b, threads=io_threads)), range(N)))
                yield [buf.ptr for buf in bufs], a, b
    finally:
        for buf in bufs:
            buf.free()
