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


def _bases(rng, n: int) -> bytes:
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _record(name: bytes, seq: bytes, width: int = 60) -> bytes:
    return b">" + name + b"\n" + b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


def long_after_short(s: int, seed: int, ragged: bool = False, k: int = 9):
    """(text, index of the long record): s reads of 12 bases (`>a\\nACGTTGCAAGGT\\n`), one record of 12 000 bases on
    60-column lines that ends inside the first 16 KiB, and a second long record that runs on into the next 16 KiB.
    ragged: every third read, never the first, is empty or shorter than k: it has no window and is a record all the same."""
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(s):
        n = 12 if not (ragged and i % 3 == 1) else (0, k - 1, 1, k - 4)[(i // 3) % 4]
        reads.append(b">a\n" + _bases(rng, n) + b"\n")
    text = b"".join(reads) + _record(b"long", _bases(rng, 12_000)) + _record(b"tail", _bases(rng, 3_000))
    return text, s


def counted_text_for(seam_text: bytes, k: int, seed: int, chunk: int = 16384, reach: int = 400) -> bytes:
    """A FASTA text to count into a table that a one-record `seam_text` is then queried against: per 16 KiB boundary of the
    seam text one record with the `reach` bases on either side of it (the ones around even boundaries twice, for counts of
    2), and one record of unrelated bases."""
    rng = np.random.default_rng(seed)
    head = seam_text.index(b"\n") + 1
    body = np.frombuffer(seam_text, dtype=np.uint8)
    is_base = body != ord("\n")
    is_base[:head] = False
    seq = body[is_base].tobytes()
    out = []
    for b in range(chunk, len(seam_text), chunk):
        at = int(is_base[:b].sum())                          # the first base of the chunk
        stretch = seq[max(at - reach, 0):at + reach]
        out.append(_record(b"around %d" % b, stretch * (2 if (b // chunk) % 2 == 0 else 1)))
    out.append(_record(b"other", _bases(rng, 20_000)))
    return b"".join(out)


def straddling_windows(seam_text: bytes, k: int, chunk: int = 16384):
    """For a one-record text of A, C, G, T and N: (start, straddles, first_base): the first base of every valid window in
    text order (the order of oracle.kmer_list); per window, the 16 KiB boundary of the text it lies across, or 0; per
    boundary, the index of the first base behind it."""
    head = seam_text.index(b"\n") + 1
    body = np.frombuffer(seam_text, dtype=np.uint8)
    is_base = body != ord("\n")
    is_base[:head] = False
    seq = body[is_base]
    bad = np.concatenate([[0], np.cumsum(seq == ord("N"))])
    start = np.flatnonzero(bad[k:] == bad[:-k])              # no N among seq[start : start + k]
    straddles, first_base = np.zeros(start.size, dtype=np.int64), {}
    for b in range(chunk, len(seam_text), chunk):
        at = first_base[b] = int(is_base[:b].sum())
        straddles[(start < at) & (start + k > at)] = b
    return start, straddles, first_base


def random_tables(k: int, n: int, seed: int) -> list:
    """n u8 tables of 4^k bytes in which 0, 1, 254 and 255 are all frequent (the edges of every count window)."""
    rng = np.random.default_rng(seed)
    pool = np.array([0, 0, 0, 1, 1, 2, 3, 17, 128, 253, 254, 254, 255, 255], dtype=np.uint8)
    return [pool[rng.integers(0, pool.size, 4 ** k)] for _ in range(n)]
