"""The yardstick of the query path: per-record k-mer hits restated on the host.

For FASTQ the text is first turned into the FASTA it stands for (fastq_ref).  oracle.kmer_list gives every canonical k-mer
of the valid windows in text order together with the records; split at the cumulative sums of n_valid_kmers they are the
windows of each record.  Per record and table: c = table[kmers]; hits = #(min <= c <= max); depth = sum of c over those."""
import functools
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


def long_after_short(s: int, seed: int, ragged: bool = False, k: int = 9, read_len: int = 12, source: bytes = None,
                     tail_len: int = 3000):
    """(text, index of the long record): s reads of read_len bases (`>a\\nACGTTGCAAGGT\\n`), one record of 12 000 bases on
    60-column lines that ends inside the first 16 KiB, and a second long record, of tail_len bases, that runs on into the
    next 16 KiB (with few reads only if it is longer than 3000 bases).
    ragged: every third read, never the first, is empty or shorter than k: it has no window and is a record all the same.
    source: a string of at least 12 000 + tail_len bases (mosaic): the two long records are its first bases and the reads are
    cut from it anywhere, so that all of them hit the tables the source was counted into; without it the bases are random."""
    rng = np.random.default_rng(seed)
    assert source is None or len(source) >= 12_000 + tail_len + read_len

    def cut(n):
        if source is None:
            return _bases(rng, n)
        at = int(rng.integers(0, len(source) - n + 1))
        return source[at:at + n]

    reads = []
    for i in range(s):
        n = read_len if not (ragged and i % 3 == 1) else (0, k - 1, 1, k - 4)[(i // 3) % 4]
        reads.append(b">a\n" + cut(n) + b"\n")
    long_, tail = (_bases(rng, 12_000), _bases(rng, tail_len)) if source is None else (source[:12_000], source[12_000:12_000 + tail_len])
    text = b"".join(reads) + _record(b"long", long_) + _record(b"tail", tail)
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


# ------------------------------------------------------------------ read-shaped input at k = 13, 15, 17
CHUNK = 16384
COUNT_WINDOWS = ((1, 255), (2, 254), (255, 255))
TANDEM_COPIES = 260                                          # > 255: every k-mer inside a tandem repeat is counted to the clip


def seam_text(k: int) -> bytes:
    """One record of 100 000 bases, line width 60 (seven 16 KiB chunks), an N within k-1 bases on either side of two chunk
    boundaries."""
    rng = np.random.default_rng(200 + k)
    seq = bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 100_000)].tobytes())
    head = b">seams one record\n"
    def base_at(byte):                                       # index of the base at (or just before) a byte offset of the text
        body = byte - len(head)
        return body - body // 61                             # 60 bases + '\n' per line
    for boundary, delta in ((2 * CHUNK, -(k - 2)), (2 * CHUNK, 1), (5 * CHUNK, -1), (5 * CHUNK, k - 2)):
        seq[base_at(boundary) + delta] = ord("N")
    body = b"".join(bytes(seq[i:i + 60]) + b"\n" for i in range(0, len(seq), 60))
    return head + body


def reads_text(k: int, n_reads: int = 6000, seed: int = 31) -> bytes:
    """`>rN\\n<bases>\\n` per read, lengths 0, 1, k-1, k, k+1, 40 ... mixed: many records per 64-byte piece and per chunk."""
    rng = np.random.default_rng(seed)
    lens = np.array([0, 1, k - 1, k, k + 1, 40, 2, 13, 64, 150])[rng.integers(0, 10, n_reads)]
    lens[:12] = [0, 0, 1, k - 1, k, k + 1, 40, 0, k, 0, 0, 1]
    alphabet = np.frombuffer(b"ACGTACGTACGTACGTN", dtype=np.uint8)
    out = []
    for i, n in enumerate(lens):
        out.append(b">r%d\n" % i + alphabet[rng.integers(0, alphabet.size, int(n))].tobytes() + b"\n")
    return b"".join(out)


def sequence(fasta: bytes) -> bytes:
    """The bases of a FASTA text whose lines end in `\\n`, record after record, headers and line ends left out."""
    return b"".join(ln for ln in fasta.split(b"\n") if not ln.startswith(b">"))


def _counted_layout(k: int, n: int, seed: int):
    """(texts, common): counted_sources' texts and, per text, (first, end) of its stretch `common x1` in sequence(text)."""
    rng = np.random.default_rng(seed)
    unit = k + 3                                             # a tandem repeat's unit is longer than k: k-mers of `unit` different phases

    def stretches(once: int, twice: int):
        return {"x1": _bases(rng, once), "x2": _bases(rng, twice), "x255": _bases(rng, unit) * TANDEM_COPIES}

    common = stretches(5000, 2000)
    shared = [stretches(3000, 1500) for _ in range(n - 1)]    # shared[i]: in table i and in table i + 1
    texts, marks = [], []
    for i in range(n):
        own = stretches(16_000, 4000)
        groups = [("own", own)] + ([("prev", shared[i - 1])] if i > 0 else []) + [("common", common)] + \
                 ([("next", shared[i])] if i < n - 1 else [])
        recs = [(b"%s %s" % (who.encode(), c.encode()), g[c]) for who, g in groups for c in ("x1", "x2", "x255")]
        recs += [(b"%s x2 again" % who.encode(), g["x2"]) for who, g in groups]
        at = sum(len(seq) for name, seq in recs[:[name for name, _ in recs].index(b"common x1")])
        marks.append((at, at + len(common["x1"])))
        texts.append(b"".join(_record(name, seq) for name, seq in recs))
    return texts, marks


def counted_sources(k: int, n: int, seed: int) -> list:
    """n FASTA texts of about 60 kbp to count into n tables.  Every text is made of random stretches that occur in it once
    (`x1`), twice (`x2`, as two records) and 260 times (`x255`: a tandem repeat of a unit of k + 3 bases, which the table
    clips to 255), so the count windows (1, 255), (2, 254) and (255, 255) select three different non-empty sets of its
    k-mers.  Per count there is a stretch of the text's own, one that all n texts hold (`common`) and one that text i shares
    with text i + 1: every pair of tables shares some of its hits under every window, and no pair all of them."""
    return _counted_layout(k, n, seed)[0]


def mosaic(sources: Sequence[bytes], n_bases: int, seed: int, piece: int = 300) -> bytes:
    """n_bases bases: pieces of `piece` bases cut from the sources' sequences, source and place at random."""
    rng = np.random.default_rng(seed)
    seqs = [sequence(s) for s in sources]
    out = []
    for _ in range(-(-n_bases // piece)):
        s = seqs[int(rng.integers(0, len(seqs)))]
        at = int(rng.integers(0, len(s) - piece + 1))
        out.append(s[at:at + piece])
    return b"".join(out)[:n_bases]


def read_lengths(k: int) -> tuple:
    return (0, 1, k - 2, k - 1, k, k + 1, 15, 16, 17, 18, 31, 32, 33, 34, 2 * k - 1, 2 * k, 64, 150)


def reads_from(sources: Sequence[bytes], k: int, n_reads: int, seed: int, fastq: bool = False) -> bytes:
    """n_reads reads `>rN\\n<bases>\\n`, lengths drawn from read_lengths(k): several records in a thread's 16 windows, reads
    without a window, reads of one window.  Six reads in seven are cut from a source's sequence (source and place at
    random), every seventh is random; every fifth non-empty read has one base replaced by N.
    fastq: the same reads as `@rN`, bases, `+`, qualities, every third record with \\r\\n line ends.  The qualities are random
    bytes in 33 .. 73; a read has none, 2 %, 10 % or half of them below 53 (33 + 20), so that masking at Q = 20 takes
    windows away and leaves others (uniform qualities would leave no window of 13 bases or more)."""
    rng, qrng = np.random.default_rng(seed), np.random.default_rng(seed + 1)
    seqs = [sequence(s) for s in sources]
    lengths = read_lengths(k)
    out, non_empty = [], 0
    for i in range(n_reads):
        n = lengths[int(rng.integers(0, len(lengths)))]
        if i % 7 == 6:
            seq = bytearray(_bases(rng, n))
        else:
            s = seqs[int(rng.integers(0, len(seqs)))]
            at = int(rng.integers(0, len(s) - n + 1))
            seq = bytearray(s[at:at + n])
        if n:
            non_empty += 1
            if non_empty % 5 == 0:
                seq[int(rng.integers(0, n))] = ord("N")
        if not fastq:
            out.append(b">r%d\n" % i + bytes(seq) + b"\n")
            continue
        low = qrng.random(n) < (0.0, 0.02, 0.1, 0.5)[int(qrng.integers(0, 4))]
        qual = np.where(low, qrng.integers(33, 53, n), qrng.integers(53, 74, n)).astype(np.uint8).tobytes()
        nl = b"\r\n" if i % 3 == 0 else b"\n"
        out.append(b"@r%d" % i + nl + bytes(seq) + nl + b"+" + nl + qual + nl)
    return b"".join(out)


def record_break_at(k: int, d: int, seed: int = 0, n: int = 2):
    """(text, sources): two records A and B in a text of two 16 KiB chunks.  B's first base is valid base number d of the
    second chunk, -k <= d <= k: for d > 0 the chunk begins with the last d bases of A (then A's line end and B's header),
    for d = 0 with B's first base, for d < 0 with base -d of B, whose first -d bases end the first chunk.  A fills the
    first chunk (its waves but the last lie wholly in A), B has 2200 bases.  Both are cut from counted_sources(k, n, seed):
    A from the first text, ending inside the stretch that both texts hold once, B from that stretch of the second, so the
    windows on either side of the break hit every table."""
    assert -k <= d <= k
    texts, marks = _counted_layout(k, n, seed)
    seq_a, seq_b = sequence(texts[0]), sequence(texts[1])
    a_bytes = CHUNK + d + 1 if d > 0 else CHUNK + d - len(b">B\n")      # `>A..\n` and A's lines, its last line end included
    for pad in range(61):                                    # A's name is padded until A's last line holds more than k bases
        body = a_bytes - len(b">A\n") - pad
        full, rest = divmod(body, 61)
        if rest == 0 or rest - 1 > k + 3:
            break
    n_a = 60 * full + max(rest - 1, 0)
    end_a = marks[0][0] + 2500
    assert end_a >= n_a and marks[0][1] - marks[0][0] >= 2500 and marks[1][1] - marks[1][0] >= 1000 + 2200
    a = _record(b"A" + b"x" * pad, seq_a[end_a - n_a:end_a])
    assert len(a) == a_bytes
    b_at = marks[1][0] + 1000
    return a + _record(b"B", seq_b[b_at:b_at + 2200]), texts


# The cases of tests/test_gpu_query_reads.py, built once; tests/test_query_host.py checks on the CPU what they rely on.
def n_tables(k: int) -> int:
    return 2 if k == 17 else 3                               # k = 17: 16 GiB a table


@functools.lru_cache(maxsize=None)
def counted_case(k: int):
    """(sources, SparseTables of them): what the GPU tests count into their tables at k, and how the reference reads them."""
    sources = tuple(counted_sources(k, n_tables(k), seed=1300 + k))
    return sources, tuple(SparseTable(oracle.kmer_list(src, k)) for src in sources)


@functools.lru_cache(maxsize=None)
def reads_case(k: int, n_reads: int = 3000, fastq: bool = False) -> bytes:
    return reads_from(counted_case(k)[0], k, n_reads, seed=1400 + k, fastq=fastq)


@functools.lru_cache(maxsize=None)
def rows_case(s: int, ragged: bool, k: int = 17):
    """long_after_short at k >= 13: reads of k + 3 bases (four windows), everything cut from a mosaic of the counted sources;
    a tail of 4000 bases reaches the second chunk behind 31 reads too."""
    source = mosaic(counted_case(k)[0], 16_100, seed=1500 + k)
    return long_after_short(s, seed=1600 + s, ragged=ragged, k=k, read_len=k + 3, source=source, tail_len=4000)


@functools.lru_cache(maxsize=None)
def break_case(k: int, d: int) -> bytes:
    """record_break_at on the counted sources of k (counted_case's seed and number of tables)."""
    text, sources = record_break_at(k, d, seed=1300 + k, n=n_tables(k))
    assert tuple(sources) == counted_case(k)[0]
    return text
