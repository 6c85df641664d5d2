"""The yardstick of the extract path: the definition (README "Extracting k-mers") on whole numpy arrays."""
import numpy as np


def select_mask(present, absent, min_count, max_count, min_present=None, max_absent=0):
    """Boolean mask over the addresses of the tables (equal-length uint8 arrays)."""
    min_present = len(present) if min_present is None else min_present
    p = np.zeros(present[0].size, dtype=np.int32)
    for t in present:
        p += (t >= min_count) & (t <= max_count)
    q = np.zeros(present[0].size, dtype=np.int32)
    for t in absent:
        q += t >= 1
    return (p >= min_present) & (q <= max_absent)


def expected(present, absent, min_count, max_count, min_present=None, max_absent=0, first_addr=0):
    """(addr (M,) uint64 ascending, counts (M, P) uint8): the selected addresses and the present tables' raw bytes there."""
    idx = np.flatnonzero(select_mask(present, absent, min_count, max_count, min_present, max_absent))
    counts = np.stack([np.asarray(t)[idx] for t in present], axis=1).astype(np.uint8).reshape(idx.size, len(present))
    return idx.astype(np.uint64) + np.uint64(first_addr), counts


def decode(addr, k):
    """(M, k + 1) uint8: the k letters of every address (codes 0,1,2,3 = A,C,G,T, first base in the highest bits: the
    inverse of the indexer's encoding) and a newline."""
    addr = np.asarray(addr, dtype=np.uint64)
    out = np.empty((addr.size, k + 1), dtype=np.uint8)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    for p in range(k):
        out[:, p] = letters[((addr >> np.uint64(2 * (k - 1 - p))) & np.uint64(3)).astype(np.int64)]
    out[:, k] = ord("\n")
    return out


def mixed_tables(n, n_tables, seed, min_count=2, max_count=200, zero=0.4):
    """n_tables uint8 arrays of n bytes: a share `zero` of zeros, the rest split between counts inside the window, just
    outside it on either side, and anything."""
    rng = np.random.default_rng(seed)
    pool = np.array([min_count, max_count, (min_count + max_count) // 2, max(min_count - 1, 1), min(max_count + 1, 255), 1, 255, 7], dtype=np.uint8)
    out = []
    for _ in range(n_tables):
        t = pool[rng.integers(0, pool.size, n)]
        t[rng.random(n) < zero] = 0
        out.append(t)
    return out
