"""Seeded FASTQ streams of the size and shape of real feeds for the trim and correct kernels (test_record_feed_inputs_host.py,
test_gpu_record_feeds.py), and their references, computed once per process and shared by both files.

The streams are built around three constants of the kernels; test_record_feed_inputs_host.py reads them out of the sources,
so a change there fails a test instead of quietly moving the seams away from these inputs:
  SCAN_ROUND = 4096   = TRIM_SCAN_T * TRIM_SCAN_PER (kmer_trim.hip): the records of one round of k_trim_scan.  From record
                        4096 of a feed on, the ordinal of a record's first cover bit holds the carry of the rounds before it.
  STRIDE     = 32 768 = TRIM_MAX_WGS * TRIM_WAVES (kmer_trim.h): the records of one pass of the capped grid of k_trim_count,
                        k_trim_runs and k_correct_runs.  From record 32 768 of a feed on, a wave takes its second record.
  ROUND      = 256    = TRIM_ROUND (kmer_trim.h): the bytes that trim_line_end and the walks of line 2 load at a time.

many(k, seed): R_MANY = 70 000 records, three passes of the grid and 18 rounds of the scan in one feed.  `\\n` line ends,
  names "r<i>", a bare '+'.  Line 2 of record i has 0 .. 2 k + 2 bases: cut from the tables' genome with one substitution
  planted when it is longer than k (even i), or random (odd i).  Every 97th record (i % 97 == 37) is LONG -- 63, 64, 65, 129
  or 257 bases in turn -- so that a wave's ring is full when it goes on to its next record; the record STRIDE behind a long
  one of 129 or 257 bases, which the same wave takes next when the feed is the whole stream, is a genome read of 2 k + 2
  bases with a substitution in the middle that is built to be corrected (_correctable).  The records b - 1, b and
  b + 1 around every multiple b of SCAN_ROUND are SEAM records: 2 k bases of the genome, which the tables cover, and behind
  them 2 k bases of which no window is in any table, so the last one is never covered: their bits are mixed whatever the
  seed.  About 3 % of the other records hold an N, about 5 % a lower-case stretch.  Qualities are random.
  many_bits(n_valid_bases, seed): cover bits for the Trimmer, independent per base with p = 0.7 (not the all / none classes
  of trim_inputs.bits, inside which a shifted ordinal could hide).
  Tables for the Corrector: correct_inputs.tables(5, 3, seed) with M = 2; its cover bits are the reference's own.

long_lines(k, seed): N_LONG = 126 records, record i with
  terminator   EOLS[(i + i // 9) % 3]
  line 1       LINE1[i % 7] bytes = 255, 256, 257, 511, 512, 513, 1000: '@' and a name with '@', '+', blanks and bytes
               >= 0x80 (with `\\r\\n` and 255 bytes the `\\r` is byte 255 of trim_line_end's first round, the `\\n` byte 256)
  line 3       '+' and the name (odd i) or a bare '+' (even i)
  line 2       BLANK_RUNS[(i // 2) % 7] leading and BLANK_RUNS[(i // 3) % 7] trailing blanks = 0, 63, 64, 65, 255, 256, 257,
               drawn from correct_inputs.BLANKS; line 4 as long
  sequence     SEQ(k)[i % 9] bases = k, 257, 511, 512, 513, 1023, 1024, 1025, 4097: 7 and 9 are coprime, so every line 1
               meets every sequence length.  Even i: cut from the genome (taken round when it is shorter than the read), with
               substitutions at every third of the positions 0, k - 1, 255 .. 257, 511 .. 513, 1023 .. 1025, n - k, n - 1
               (which third: (i // 18) % 3, the read's number among the genome reads of its length, so that every length
               gets every third and no two substitutions share a window), and for every second such read one more k - 1
               or k behind one of them, as correct_inputs.stream does.  Odd i: random.  i % 5 == 0: a lower-case stretch,
               i % 7 == 0: one or two Ns.
  Record 60 is followed by one more: GIANT = 40 000 bases of the genome with 1 % substitutions, 157 rounds of 256.
  The last record has no final terminator.
  Its tables are correct_inputs.tables(k, 3, seed, density=long_density(k)).  At the default density of one half a substituted
  base of a long read is nearly always covered by a chance match (it stays uncovered with probability 2^-k), and long reads
  would hold hardly any candidate.  long_density(k) = 1 - UNCOVERED^(1 / k) makes it a candidate with probability UNCOVERED =
  0.45 at every k: about 90 of the 200 substitutions behind position 20 000 of the giant read, and corrected unless a
  neighbour interferes.

Reference times on the CPU (one core): many at k = 5 about 5 s for correct_ref.expected and 3 s for trim_ref.runs, the same
again under the threshold; long_lines about 2.5 s per correct_ref.expected and 0.3 s per trim_ref.runs; the three k = 13
tables (64 MiB each) take about 1 s to count and fill, and the k = 13 reference is no slower than the others.
"""
import functools

import numpy as np

import correct_inputs
import correct_ref
import fastq_qual_ref
import mask_ref
import trim_ref
from correct_inputs import BLANKS, EOLS, LETTERS

SCAN_ROUND = 4096
STRIDE = 32768
ROUND = 256
R_MANY = 70_000
LONG = (63, 64, 65, 129, 257)
LINE1 = (255, 256, 257, 511, 512, 513, 1000)
BLANK_RUNS = (0, 63, 64, 65, 255, 256, 257)
N_LONG = 126
GIANT = 40_000
GIANT_AFTER = 60
UNCOVERED = 0.45
T = 53                                                       # the threshold byte of --min-qual 20 at offset 33
K_MANY = 5


def SEQ(k: int):
    return (k, 257, 511, 512, 513, 1023, 1024, 1025, 4097)


def long_density(k: int) -> float:
    return 1.0 - UNCOVERED ** (1.0 / k)


def seams(R: int = R_MANY):
    """The multiples of SCAN_ROUND below R (STRIDE and 2 * STRIDE are among them)."""
    return list(range(SCAN_ROUND, R, SCAN_ROUND))


def is_long(i: int) -> int:
    """The bases of record i of many() if it is a long one, else 0."""
    return LONG[(i // 97) % len(LONG)] if i % 97 == 37 else 0


def _cut(source: np.ndarray, n: int, rng) -> np.ndarray:
    """n consecutive bases of the genome from a random place, taken round when the genome is shorter."""
    at = int(rng.integers(0, source.size))
    return source[(at + np.arange(n)) % source.size].copy() if at + n > source.size else source[at:at + n].copy()


def _absent_tail(k: int, tabs, rng) -> np.ndarray:
    """2 k bases of which no window is in any table."""
    while True:
        codes = rng.integers(0, 4, 2 * k)
        addrs = [correct_ref.address(codes[s:s + k].tolist()) for s in range(k + 1)]
        if not any(int(t[a]) for t in tabs for a in addrs):
            return LETTERS[codes].copy()


def _correctable(k: int, tabs, source: np.ndarray, rng) -> np.ndarray:
    """2 k + 2 bases of one table's genome with a substitution at position k + 1 that is a candidate with k windows -- none of
    them in any table -- and which only the genome's own base mends."""
    p = k + 1
    while True:
        at = int(rng.integers(0, source.size - (2 * k + 2) + 1))
        codes = [correct_ref.CODE[c] for c in source[at:at + 2 * k + 2].tolist()]

        def held(b):
            """How many of the k windows over p are in a table with base b at p."""
            row = codes[:p] + [b] + codes[p + 1:]
            return sum(any(int(t[correct_ref.address(row[s:s + k])]) for t in tabs) for s in range(p - k + 1, p + 1))
        others = [b for b in range(4) if b != codes[p]]
        rng.shuffle(others)
        if held(others[0]) == 0 and held(others[1]) < k and held(others[2]) < k:
            codes[p] = others[0]
            return LETTERS[np.array(codes)].copy()


def many(k: int, seed: int, R: int = R_MANY) -> bytes:
    tabs, genome = many_tables(k)
    rng = np.random.default_rng(seed)
    source = np.frombuffer(genome, dtype=np.uint8)
    seam = {b + d for b in seams(R) for d in (-1, 0, 1)}
    tail = _absent_tail(k, tabs, rng)
    mendable = [_correctable(k, tabs, source[:source.size // 3], rng) for _ in range(16)]
    lengths = rng.integers(0, 2 * k + 3, R)
    dice = rng.random(R)
    recs = []
    for i in range(R):
        n = int(lengths[i])
        plain = False
        if i in seam:
            at = int(rng.integers(0, source.size // 3 - 2 * k + 1))                       # inside the first table's genome
            seq = np.concatenate([source[at:at + 2 * k], tail])
            plain = True
        else:
            n = is_long(i) or n
            if not is_long(i) and i >= STRIDE and is_long(i - STRIDE) >= 129:
                seq, plain = mendable[i % len(mendable)].copy(), True
            elif i % 2 == 0:
                seq = _cut(source, n, rng)
                if n > k:
                    correct_inputs._substitute(seq, int(rng.integers(0, n)), rng)
            else:
                seq = LETTERS[rng.integers(0, 4, n)].copy()
        if n and not plain:
            if dice[i] < 0.03:
                seq[int(rng.integers(0, n))] = ord("N")
            elif dice[i] < 0.08:
                a = int(rng.integers(0, n))
                seq[a:a + 6] |= 0x20
        qual = rng.integers(33, 127, size=seq.size).astype(np.uint8)
        recs.append(b"@r%d\n" % i + seq.tobytes() + b"\n+\n" + qual.tobytes() + b"\n")
    return b"".join(recs)


def many_bits(n_valid_bases, seed: int, p: float = 0.7) -> np.ndarray:
    """(sum of n_valid_bases,) bool: every bit set with probability p, independently."""
    return np.random.default_rng(seed).random(int(np.asarray(n_valid_bases).sum())) < p


def _name(length: int, i: int, rng) -> bytes:
    """`length` name bytes, none a line terminator: letters with '@', '+', blanks and bytes >= 0x80 among them."""
    pool = np.frombuffer(b"abcXYZ019_/:.@+ \t\x0b\x1c\x1f\x80\xa5\xc3\xa9\xff", dtype=np.uint8)
    body = pool[rng.integers(0, pool.size, length)].tobytes()
    head = b"r%d @+ \t\x80\xff" % i
    return (head + body[len(head):])[:length]


def _blank(m: int, rng) -> bytes:
    return bytes(BLANKS[int(b)] for b in rng.integers(0, len(BLANKS), size=m))


def planted(k: int, n: int):
    """The positions of a read of n bases at which long_lines plants substitutions, a third of them per read."""
    near = [p for c in (256, 512, 1024) for p in (c - 1, c, c + 1)]
    return sorted({p for p in [0, k - 1, n - k, n - 1] + near if 0 <= p < n})


def long_lines(k: int, seed: int) -> bytes:
    genome = long_tables(k)[1]
    rng = np.random.default_rng(seed)
    source = np.frombuffer(genome, dtype=np.uint8)
    recs = []
    for i in range(N_LONG):
        eol = EOLS[(i + i // 9) % 3]
        n = SEQ(k)[i % 9]
        if i % 2 == 0:
            j = i // 18                                      # the j-th genome read of this length
            seq = _cut(source, n, rng)
            spots = planted(k, n)[j % 3::3]
            for p in spots:
                correct_inputs._substitute(seq, p, rng)
            if j % 2 == 0 and spots:                         # a second error k - 1 or k behind the middle one
                p = spots[len(spots) // 2] + (k - 1, k)[(j // 2) % 2]
                if p < n and all(abs(p - s) > k for s in spots if s != spots[len(spots) // 2]):
                    correct_inputs._substitute(seq, p, rng)
        else:
            seq = LETTERS[rng.integers(0, 4, n)].copy()
        if i % 5 == 0:
            a = int(rng.integers(0, n))
            seq[a:a + 20] |= 0x20
        if i % 7 == 0:
            seq[rng.integers(0, n, size=int(rng.integers(1, 3)))] = ord("N")
        line2 = _blank(BLANK_RUNS[(i // 2) % 7], rng) + seq.tobytes() + _blank(BLANK_RUNS[(i // 3) % 7], rng)
        name = _name(LINE1[i % 7] - 1, i, rng)
        qual = rng.integers(33, 127, size=len(line2)).astype(np.uint8)
        recs.append(b"@" + name + eol + line2 + eol + b"+" + (name if i % 2 else b"") + eol + qual.tobytes() + eol)
        if i == GIANT_AFTER:
            seq = _cut(source, GIANT, rng)
            for p in np.flatnonzero(rng.random(GIANT) < 0.01).tolist():
                correct_inputs._substitute(seq, p, rng)
            recs.append(b"@giant\n" + seq.tobytes() + b"\n+\n" + rng.integers(33, 127, size=GIANT).astype(np.uint8).tobytes() + b"\n")
    data = b"".join(recs)
    return data[:-len(EOLS[(N_LONG - 1 + (N_LONG - 1) // 9) % 3])]


# ------------------------------------------------------------------ the cases: inputs and references, computed once
@functools.lru_cache(maxsize=None)
def many_tables(k: int = K_MANY):
    return correct_inputs.tables(k, 3, seed=900 + k)


@functools.lru_cache(maxsize=None)
def long_tables(k: int):
    return correct_inputs.tables(k, 3, seed=920 + k, density=long_density(k))


@functools.lru_cache(maxsize=None)
def many_stream(tq: int = 0) -> bytes:
    fq = many(K_MANY, seed=910)
    return fastq_qual_ref.biased_qualities(fq, tq, 0.1, seed=7) if tq else fq


@functools.lru_cache(maxsize=None)
def many_starts(tq: int = 0) -> np.ndarray:
    return trim_ref.starts(many_stream(tq))


@functools.lru_cache(maxsize=None)
def many_correct(tq: int = 0) -> dict:
    """correct_ref.expected of the many-record stream: k = 5, the three tables, M = 2."""
    return correct_ref.expected(many_stream(tq), K_MANY, many_tables()[0], M=2, T=tq)


@functools.lru_cache(maxsize=None)
def many_trim(tq: int = 0) -> dict:
    """trim_ref.runs of the many-record stream under many_bits; "bits": the packed cover bits."""
    fq = many_stream(tq)
    base_rec = mask_ref.walk_fast(trim_ref.fasta_of(fq, tq), 1)[1]
    cover = many_bits(np.bincount(base_rec, minlength=len(many_starts(tq)) - 1), seed=911 + tq)
    want = trim_ref.runs(fq, cover, T=tq)
    want["bits"] = mask_ref.pack(cover)
    return want


@functools.lru_cache(maxsize=None)
def long_stream(k: int) -> bytes:
    return long_lines(k, seed=930 + k)


@functools.lru_cache(maxsize=None)
def long_starts(k: int) -> np.ndarray:
    return trim_ref.starts(long_stream(k))


@functools.lru_cache(maxsize=None)
def long_correct(k: int, M=None) -> dict:
    return correct_ref.expected(long_stream(k), k, long_tables(k)[0], M=M)


@functools.lru_cache(maxsize=None)
def long_trim(k: int) -> dict:
    fq = long_stream(k)
    base_rec = mask_ref.walk_fast(trim_ref.fasta_of(fq), 1)[1]
    cover = many_bits(np.bincount(base_rec, minlength=len(long_starts(k)) - 1), seed=940 + k)
    want = trim_ref.runs(fq, cover)
    want["bits"] = mask_ref.pack(cover)
    return want
