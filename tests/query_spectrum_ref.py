"""The yardstick of the query's count spectra: the definition restated on the host, independently of the kernels.

oracle.kmer_list gives the canonical k-mers of all valid windows in text order and the records.  A window belongs to the row
its ordinal falls in: record r for the ordinals [cumsum(n_valid)[r], cumsum(n_valid)[r + 1]), or, with bins of W windows,
the row of query_bins_ref.bin_bounds.  spectrum[row][t][c] = the number of the row's windows whose k-mer has T_t[kmer] == c."""
from typing import Sequence

import numpy as np

import oracle
import query_bins_ref
from fastq_ref import fastq_to_fasta


def expected(text: bytes, k: int, tables: Sequence, W: int = None, fmt: str = "fasta") -> dict:
    """dict(records, fasta, n_valid (R,), seq_len (R,), spectrum (rows, N, 256) uint64, median (rows, N) uint8, row_windows
    (rows,)[, bin_first (R + 1,)]): the rows are the records, or with W the bins.  `tables`: u8 arrays of 4^k or SparseTables."""
    fasta = fastq_to_fasta(text) if fmt == "fastq" else text
    kmers, info = oracle.kmer_list(fasta, k, records=True)
    recs = info["records"]
    n_valid = recs["n_valid_kmers"].astype(np.uint64)
    assert int(n_valid.sum()) == kmers.size
    out = {"records": recs, "fasta": fasta, "n_valid": n_valid, "seq_len": recs["seq_len"].astype(np.uint64)}
    if W is None:
        row_windows = n_valid.astype(np.int64)
    else:
        bin_first, lo, hi, _, _ = query_bins_ref.bin_bounds(n_valid, W)
        assert np.array_equal(lo[1:], hi[:-1]) and (lo.size == 0 or (lo[0] == 0 and hi[-1] == kmers.size))   # the rows tile the window list
        row_windows = hi - lo
        out["bin_first"] = bin_first
    row = np.repeat(np.arange(row_windows.size, dtype=np.int64), row_windows)
    spec = np.zeros((row_windows.size, len(tables), 256), dtype=np.uint64)
    for t, table in enumerate(tables):
        np.add.at(spec[:, t, :], (row, np.asarray(table[kmers]).astype(np.int64)), 1)
    out.update(spectrum=spec, median=median(spec), row_windows=row_windows)
    return out


def median(spec: np.ndarray) -> np.ndarray:
    """Brute force: expand every spectrum into its sorted list of counts and take element (m - 1) // 2; 0 for an empty one."""
    flat = spec.reshape(-1, 256)
    out = np.zeros(flat.shape[0], dtype=np.uint8)
    for i, s in enumerate(flat):
        counts = np.repeat(np.arange(256), s.astype(np.int64))
        if counts.size:
            out[i] = counts[(counts.size - 1) // 2]
    return out.reshape(spec.shape[:-1])


def window(spec: np.ndarray, min_count: int, max_count: int):
    """(hits, depth) of a count window, by a loop over the counts."""
    hits, depth = np.zeros(spec.shape[:-1], dtype=np.uint64), np.zeros(spec.shape[:-1], dtype=np.uint64)
    for c in range(min_count, max_count + 1):
        hits += spec[..., c]
        depth += np.uint64(c) * spec[..., c]
    return hits, depth


def record_sums(spec: np.ndarray, bin_first: np.ndarray) -> np.ndarray:
    """Per-record sums of binned spectra, by a loop."""
    out = np.zeros((bin_first.size - 1,) + spec.shape[1:], dtype=np.uint64)
    for r in range(bin_first.size - 1):
        out[r] = spec[int(bin_first[r]):int(bin_first[r + 1])].sum(axis=0, dtype=np.uint64)
    return out


def check_identities(spec: np.ndarray, row_windows, hits: np.ndarray, depth: np.ndarray, min_count: int, max_count: int) -> None:
    """The identities every run must satisfy: a row's spectrum sums to its windows for every table, and the count window of
    the run, taken from the spectrum, gives the run's own hits and depth."""
    assert spec.dtype == np.uint64 and spec.shape == hits.shape + (256,) and depth.shape == hits.shape
    sums = spec.sum(axis=-1, dtype=np.uint64)
    assert np.array_equal(sums, np.broadcast_to(np.asarray(row_windows, dtype=np.uint64)[:, None], sums.shape)), "a spectrum does not sum to its windows"
    h, d = window(spec, min_count, max_count)
    assert np.array_equal(h, hits), np.argwhere(h != hits)[:5]
    assert np.array_equal(d, depth), np.argwhere(d != depth)[:5]
