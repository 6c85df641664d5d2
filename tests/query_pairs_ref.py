"""The yardstick of the query's shared windows: the definition restated on the host, independently of the kernels.

oracle.kmer_list gives the canonical k-mers of all valid windows in text order and the records.  A row is a record -- the
ordinals [cumsum(n_valid)[r], cumsum(n_valid)[r + 1]) -- or, with bins of W windows, a row of query_bins_ref.bin_bounds.
V_t(j) = (min <= T_t[kmer_j] <= max); per pair of tables i < j the cumulative sum of V_i & V_j, differenced at the row
bounds, is shared[row][p], and the cumulative sum of V_t alone is hits[row][t]."""
from typing import Sequence

import numpy as np

import oracle
import query_bins_ref
from fastq_ref import fastq_to_fasta


def pair_list(N: int):
    """The pairs i < j, row-major: (0,1) (0,2) .. (0,N-1) (1,2) .."""
    return [(i, j) for i in range(N) for j in range(i + 1, N)]


def expected(text: bytes, k: int, tables: Sequence, min_count: int, max_count: int, W: int = None, fmt: str = "fasta") -> dict:
    """dict(records, fasta, n_valid (R,), seq_len (R,), hits (rows, N), shared (rows, P), pairs (P, 2), row_windows (rows,)
    [, bin_first (R + 1,)]): the rows are the records, or with W the bins.  `tables`: u8 arrays of 4^k or SparseTables."""
    fasta = fastq_to_fasta(text) if fmt == "fastq" else text
    kmers, info = oracle.kmer_list(fasta, k, records=True)
    recs = info["records"]
    n_valid = recs["n_valid_kmers"].astype(np.uint64)
    assert int(n_valid.sum()) == kmers.size
    out = {"records": recs, "fasta": fasta, "n_valid": n_valid, "seq_len": recs["seq_len"].astype(np.uint64)}
    if W is None:
        bounds = np.concatenate([[0], np.cumsum(n_valid)]).astype(np.int64)
        lo, hi = bounds[:-1], bounds[1:]
    else:
        bin_first, lo, hi, _, _ = query_bins_ref.bin_bounds(n_valid, W)
        out["bin_first"] = bin_first
    N = len(tables)
    inside = []
    for table in tables:
        c = np.asarray(table[kmers]).astype(np.int64)
        inside.append((c >= min_count) & (c <= max_count))

    def rows_of(flags):
        cum = np.concatenate([[0], np.cumsum(flags)]).astype(np.uint64)
        return cum[hi] - cum[lo]

    pairs = pair_list(N)
    hits = np.zeros((lo.size, N), dtype=np.uint64)
    shared = np.zeros((lo.size, len(pairs)), dtype=np.uint64)
    for t in range(N):
        hits[:, t] = rows_of(inside[t])
    for p, (i, j) in enumerate(pairs):
        shared[:, p] = rows_of(inside[i] & inside[j])
    out.update(hits=hits, shared=shared, pairs=np.array(pairs, dtype=np.int32).reshape(-1, 2), row_windows=(hi - lo).astype(np.int64))
    return out


def record_sums(rows: np.ndarray, bin_first: np.ndarray) -> np.ndarray:
    """Per-record sums of binned rows, by a loop."""
    out = np.zeros((bin_first.size - 1,) + rows.shape[1:], dtype=np.uint64)
    for r in range(bin_first.size - 1):
        out[r] = rows[int(bin_first[r]):int(bin_first[r + 1])].sum(axis=0, dtype=np.uint64)
    return out


def check_identities(shared: np.ndarray, hits: np.ndarray) -> None:
    """What every run must satisfy whatever the tables are: shared[row][p] <= min(hits[row][i], hits[row][j])."""
    assert shared.dtype == np.uint64 and shared.ndim == 2 and shared.shape[0] == hits.shape[0]
    pairs = pair_list(hits.shape[1])
    assert shared.shape[1] == len(pairs)
    for p, (i, j) in enumerate(pairs):
        assert (shared[:, p] <= np.minimum(hits[:, i], hits[:, j])).all(), (p, i, j)
