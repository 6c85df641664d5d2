"""Seeded tables and FASTQ streams for the correct tests (test_correct_host.py, test_gpu_correct.py).

tables(k, n, seed) are small dense tables in which about HALF of the canonical addresses are zero in all of them
(query_ref.random_tables is 78 % full per table and leaves candidates only at the ends of reads): table t holds the k-mers of
a random genome of its own, sized so that the n of them together fill half, with counts drawn from 1, 2, 3, 254 and 255 so
that the count windows (1, 255) and (2, 254) differ.

stream(k, genome, seed) is in the style of trim_inputs.stream: reads cut from the genomes' text (every second one) or random
(the others), of the lengths at which kmer_correct.hip's 64-position steps and its one-step delay change -- 0, 1, k - 1, k,
k + 1, 2 k - 1, 63, 64, 65, 127, 128, 129, 255, 256, 257 -- with each of the three line terminators, blanks in front of, inside
and behind the sequence, Ns, lower case, substitutions planted at the positions 0, k - 1, L - k, L - 1, 62 .. 65 and
254 .. 257, pairs of substitutions k - 1 and k apart, a missing final newline or a tail of blank lines.

random_reads(n, length, seed) are the 300 x 80 reads of the class counts in test_correct_host.py.
"""
import math

import numpy as np

import oracle

BLANKS = b" \t\x0b\x0c\x1c\x1d\x1e\x1f"
EOLS = (b"\n", b"\r\n", b"\r")
POOL = np.array([1, 1, 2, 3, 254, 255], dtype=np.uint8)
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def lengths(k: int):
    return (0, 1, k - 1, k, k + 1, 2 * k - 1, 63, 64, 65, 127, 128, 129, 255, 256, 257)


def planted(k: int, n: int):
    """The positions of a read of n bases at which a substitution is planted, one of them per read."""
    return sorted({p for p in (0, k - 1, n - k, n - 1, 62, 63, 64, 65, 254, 255, 256, 257) if 0 <= p < n})


def tables(k: int, n: int, seed: int, density: float = 0.5):
    """(n u8 tables of 4^k bytes, the genomes' bases joined): together the tables hold about `density` of the canonical
    addresses."""
    rng = np.random.default_rng(seed)
    canonical = 4 ** k // 2
    per_table = 1.0 - (1.0 - density) ** (1.0 / n)
    bases = max(k, int(round(-math.log(1.0 - per_table) * canonical)))
    out, genomes = [], []
    for _ in range(n):
        genome = LETTERS[rng.integers(0, 4, bases)].tobytes()
        table = oracle.count_fasta(b">g\n" + genome + b"\n", k)["table"].copy()
        held = np.flatnonzero(table)
        table[held] = POOL[rng.integers(0, POOL.size, held.size)]
        out.append(table)
        genomes.append(genome)
    return out, b"".join(genomes)


def _substitute(seq: np.ndarray, at: int, rng) -> None:
    others = [c for c in b"ACGT" if c != (seq[at] & 0xDF)]
    seq[at] = others[int(rng.integers(0, 3))] | (seq[at] & 0x20)


def stream(k: int, genome: bytes, seed: int, reps: int = 8, final_newline: bool = True, blank_tail: bool = False) -> bytes:
    rng = np.random.default_rng(seed)
    source = np.frombuffer(genome, dtype=np.uint8)
    assert source.size >= 257
    order = [n for _ in range(reps) for n in lengths(k)]
    recs = []
    for i, j in enumerate(rng.permutation(len(order))):
        n = order[int(j)]
        eol = EOLS[i % 3]
        if i % 2 == 0:
            at = int(rng.integers(0, source.size - n + 1))
            seq = source[at:at + n].copy()
        else:
            seq = LETTERS[rng.integers(0, 4, n)].copy()
        spots = planted(k, n)
        if spots and i % 2 == 0:
            p = spots[(i // 2) % len(spots)]
            _substitute(seq, p, rng)
            gap = (k - 1, k)[(i // 2) % 2]                   # every third such read: a second error k - 1 or k bases on
            if (i // 2) % 3 == 0 and p + gap < n:
                _substitute(seq, p + gap, rng)
        if n and i % 5 == 0:                                 # a stretch of lower case
            a = int(rng.integers(0, n))
            seq[a:a + 20] |= 0x20
        if n and i % 7 == 0:                                 # one or two Ns
            seq[rng.integers(0, n, size=int(rng.integers(1, 3)))] = ord("N")
        style = i % 4                                        # 0 plain, 1 blanks in front, 2 behind, 3 in front, inside and behind
        if style == 3 and n >= 3 and i % 8 == 3:
            seq[int(rng.integers(1, n - 1))] = BLANKS[int(rng.integers(0, len(BLANKS)))]
        blank = lambda m: bytes(BLANKS[int(b)] for b in rng.integers(0, len(BLANKS), size=m))   # noqa: E731
        line2 = (blank(int(rng.integers(1, 4))) if style in (1, 3) else b"") + seq.tobytes() + (blank(int(rng.integers(1, 4))) if style in (2, 3) else b"")
        qual = rng.integers(33, 127, size=len(line2)).astype(np.uint8)
        name = b"r%d len=%d" % (i, n)
        recs.append(b"@" + name + eol + line2 + eol + b"+" + (name if i % 5 == 0 else b"") + eol + qual.tobytes() + eol)
    data = b"".join(recs)
    if not final_newline:
        data = data[:-len(EOLS[(len(order) - 1) % 3])]
    if blank_tail:
        data += b"\n\r\n\n"
    return data


def random_reads(n_reads: int, length: int, seed: int) -> bytes:
    """n_reads reads of `length` random bases, `\\n` line ends."""
    rng = np.random.default_rng(seed)
    return b"".join(b"@r%d\n" % i + LETTERS[rng.integers(0, 4, length)].tobytes() + b"\n+\n" + b"I" * length + b"\n" for i in range(n_reads))


def plant(fq: bytes, rate: float, seed: int):
    """`fq` (reads of A, C, G, T on `\\n` line ends) with substitutions planted at `rate` per base: (the new text, the byte
    offsets of the planted bases, their bytes before)."""
    rng = np.random.default_rng(seed)
    out = np.frombuffer(fq, dtype=np.uint8).copy()
    offs, olds = [], []
    pos = 0
    for i, line in enumerate(bytes(fq).split(b"\n")):
        if i % 4 == 1:
            body = line.rstrip(b"\r")
            for p in np.flatnonzero(rng.random(len(body)) < rate).tolist():
                if out[pos + p] in b"ACGT":
                    offs.append(pos + p)
                    olds.append(int(out[pos + p]))
                    _substitute(out[pos:pos + len(body)], p, rng)
        pos += len(line) + 1
    return out.tobytes(), np.array(offs, dtype=np.int64), np.array(olds, dtype=np.uint8)
