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


TILE = 4096                                                  # addresses whose count rows the write kernel emits as one byte range


def tile_ranges(mask, P, tile=TILE):
    """(g0, g1) int64 arrays, one entry per `tile` addresses of the selection mask: the bytes [g0, g1) of the (M, P) count
    array that hold the tile's rows, g0 = P * (selected addresses before the tile)."""
    per = np.add.reduceat(np.asarray(mask, dtype=np.int64), np.arange(0, len(mask), tile))
    rank = np.concatenate([[0], np.cumsum(per)[:-1]])
    return rank * P, (rank + per) * P


def sparse_tiles(per_tile, P, seed, last=17, tile=TILE):
    """(present, absent, mask): P present tables of random counts 1..255 and one absent table that is 0 at per_tile[i]
    addresses of tile i and 1..255 elsewhere, over len(per_tile) - 1 whole tiles and a last one of `last` addresses.  With
    the window 1..255, min_present = P and max_absent = 0 the selection is exactly where the absent table is 0.  A tile's
    first or last address is taken first (the first in even tiles), then the other, then inner ones."""
    rng = np.random.default_rng(seed)
    n = (len(per_tile) - 1) * tile + last
    present = [rng.integers(1, 256, n).astype(np.uint8) for _ in range(P)]
    absent = rng.integers(1, 256, n).astype(np.uint8)
    for i, c in enumerate(per_tile):
        size = min(tile, n - i * tile)
        inner = 1 + rng.choice(size - 2, size=max(c - 2, 0), replace=False)
        ends = [0, size - 1] if i % 2 == 0 else [size - 1, 0]
        at = np.concatenate([ends[:c], inner]).astype(np.int64)
        absent[i * tile + at] = 0
    return present, [absent], absent == 0


ROW_WIDTH_SEEDS = {3: 103, 5: 105, 6: 106, 7: 107, 9: 109, 127: 231}   # chosen so that row_width_case reaches every residue


def row_width_case(P):
    """(present, absent, residues): P present tables and one absent one from mixed_tables, to be selected with the window
    2..200, min_present = 1 and max_absent = 0, over 16 whole tiles and 17 addresses (P = 127: 4 tiles and 17, the fewest
    tile starts that can reach four residues); residues = the values g0 % 4 takes over the tiles."""
    n = (4 if P == 127 else 16) * TILE + 17
    tables = mixed_tables(n, P + 1, seed=ROW_WIDTH_SEEDS[P])
    g0, g1 = tile_ranges(select_mask(tables[:P], tables[P:], 2, 200, 1, 0), P)
    assert (g1 > g0).all()
    return tables[:P], tables[P:], set((g0 % 4).tolist())


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
