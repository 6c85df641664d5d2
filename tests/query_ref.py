"""The yardstick of the query path: per-record k-mer hits restated on the host.

For FASTQ the text is first turned into the FASTA it stands for (fastq_ref).  oracle.kmer_list gives every canonical k-mer
of the valid windows in text order together with the records; split at the cumulative sums of n_valid_kmers they are the
windows of each record.  Per record and table: c = table[kmers]; hits = #(min <= c <= max); depth = sum of c over those."""
from typing import Sequence

import numpy as np

import oracle
from fastq_ref import fastq_to_fasta


class SparseTable:
    """A 4^k-byte count table known only where it is non-zero (k = 17: 16 GiB): built from the k-mer list of the text that
    was counted into it -- np.unique, counts clipped to 255 -- and read by searchsorted."""

    def __init__(self, counted_kmers: np.ndarray):
        self.keys, counts = np.unique(np.asarray(counted_kmers, dtype=np.uint64), return_counts=True)
        self.vals = np.minimum(counts, 255).astype(np.uint8)

    def __getitem__(self, kmers: np.ndarray) -> np.ndarray:
        kmers = np.asarray(kmers, dtype=np.uint64)
        if self.keys.size == 0:
            return np.zeros(kmers.size, dtype=np.uint8)
        at = np.minimum(np.searchsorted(self.keys, kmers), self.keys.size - 1)
        return np.where(self.keys[at] == kmers, self.vals[at], 0).astype(np.uint8)


def expected(text: bytes, k: int, tables: Sequence, min_count: int, max_count: int, fmt: str = "fasta") -> dict:
    """dict(records, n_valid (R,), seq_len (R,), hits (R, N), depth (R, N)), uint64; `tables`: u8 arrays of 4^k or SparseTables."""
    fasta = fastq_to_fasta(text) if fmt == "fastq" else text
    kmers, info = oracle.kmer_list(fasta, k, records=True)
    recs = info["records"]
    n_valid = recs["n_valid_kmers"].astype(np.uint64)
    bounds = np.concatenate([[0], np.cumsum(n_valid)]).astype(np.int64)
    assert bounds[-1] == kmers.size
    R, N = len(recs), len(tables)
    hits, depth = np.zeros((R, N), dtype=np.uint64), np.zeros((R, N), dtype=np.uint64)
    for t, table in enumerate(tables):
        c = np.asarray(table[kmers]).astype(np.uint64)
        inside = (c >= min_count) & (c <= max_count)
        cum_h = np.concatenate([[0], np.cumsum(inside)]).astype(np.uint64)
        cum_d = np.concatenate([[0], np.cumsum(np.where(inside, c, 0))]).astype(np.uint64)
        hits[:, t] = cum_h[bounds[1:]] - cum_h[bounds[:-1]]
        depth[:, t] = cum_d[bounds[1:]] - cum_d[bounds[:-1]]
    return {"records": recs, "fasta": fasta, "n_valid": n_valid, "seq_len": recs["seq_len"].astype(np.uint64), "hits": hits, "depth": depth}


def names(fasta: bytes, recs) -> list:
    return [fasta[int(r["name_off"]):int(r["name_off"]) + int(r["name_len"])].decode("utf-8", "replace") for r in recs]


def random_tables(k: int, n: int, seed: int) -> list:
    """n u8 tables of 4^k bytes in which 0, 1, 254 and 255 are all frequent (the edges of every count window)."""
    rng = np.random.default_rng(seed)
    pool = np.array([0, 0, 0, 1, 1, 2, 3, 17, 128, 253, 254, 254, 255, 255], dtype=np.uint8)
    return [pool[rng.integers(0, pool.size, 4 ** k)] for _ in range(n)]
