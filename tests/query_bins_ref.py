"""The yardstick of binned query hits: the definition restated on the host, independently of the kernels.

Record r has m = n_valid[r] valid windows, numbered j = 0 .. m-1 in text order, and ceil(m / W) bins; bin b holds the windows
b*W <= j < min((b+1)*W, m).  Rows are ordered by record, then by bin; bin_first[r] is record r's first row and bin_first[R]
the number of rows.  oracle.kmer_list gives the canonical k-mers of all valid windows in text order, so window j of record r
is entry cumsum(n_valid)[r] + j of that list: cumulative sums of "inside the count window" and of the counts, differenced at
the bin boundaries, are the rows."""
from typing import Sequence

import numpy as np

import oracle
from fastq_ref import fastq_to_fasta


def bin_bounds(n_valid: np.ndarray, W: int):
    """(bin_first (R+1,), lo (B,), hi (B,), record (B,), bin (B,)): row i covers entries [lo[i], hi[i]) of the window list."""
    n_valid = np.asarray(n_valid, dtype=np.int64)
    assert int(W) >= 1
    W = min(int(W), 1 << 40)                                 # beyond any m the bins are the same: one per record with a window
    n_bins = -(-n_valid // W)                                # ceil; 0 for a record without a window
    bin_first = np.concatenate([[0], np.cumsum(n_bins)]).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(n_valid)]).astype(np.int64)
    record = np.repeat(np.arange(n_valid.size, dtype=np.int64), n_bins)
    b = np.arange(bin_first[-1], dtype=np.int64) - bin_first[record]
    lo = start[record] + b * W
    hi = np.minimum(lo + W, start[record + 1])
    return bin_first.astype(np.uint64), lo, hi, record, b


def expected(text: bytes, k: int, tables: Sequence, min_count: int, max_count: int, W: int, fmt: str = "fasta") -> dict:
    """dict(records, fasta, n_valid (R,), seq_len (R,), hits (R, N), depth (R, N), bin_hits (B, N), bin_depth (B, N),
    bin_first (R+1,), row_record (B,), row_bin (B,), row_windows (B,)); integer arrays uint64 but the three row_* (int64).
    `tables`: u8 arrays of 4^k or query_ref.SparseTables."""
    fasta = fastq_to_fasta(text) if fmt == "fastq" else text
    kmers, info = oracle.kmer_list(fasta, k, records=True)
    recs = info["records"]
    n_valid = recs["n_valid_kmers"].astype(np.uint64)
    rec_bounds = np.concatenate([[0], np.cumsum(n_valid)]).astype(np.int64)
    assert rec_bounds[-1] == kmers.size
    bin_first, lo, hi, record, b = bin_bounds(n_valid, W)
    assert np.all(hi > lo) and np.all(hi - lo <= W)           # no empty row
    R, B, N = len(recs), lo.size, len(tables)
    out = {key: np.zeros(shape, dtype=np.uint64) for key, shape in
           (("hits", (R, N)), ("depth", (R, N)), ("bin_hits", (B, N)), ("bin_depth", (B, N)))}
    for t, table in enumerate(tables):
        c = np.asarray(table[kmers]).astype(np.uint64)
        inside = (c >= min_count) & (c <= max_count)
        cum_h = np.concatenate([[0], np.cumsum(inside)]).astype(np.uint64)
        cum_d = np.concatenate([[0], np.cumsum(np.where(inside, c, 0))]).astype(np.uint64)
        out["hits"][:, t] = cum_h[rec_bounds[1:]] - cum_h[rec_bounds[:-1]]
        out["depth"][:, t] = cum_d[rec_bounds[1:]] - cum_d[rec_bounds[:-1]]
        out["bin_hits"][:, t] = cum_h[hi] - cum_h[lo]
        out["bin_depth"][:, t] = cum_d[hi] - cum_d[lo]
    out.update(records=recs, fasta=fasta, n_valid=n_valid, seq_len=recs["seq_len"].astype(np.uint64), bin_first=bin_first,
               row_record=record, row_bin=b, row_windows=hi - lo)
    return out
