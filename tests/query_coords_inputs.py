"""The query texts of the coordinate tests (test_gpu_query_coords.py; test_query_coords_host.py ties the yardstick to the
oracle on the same texts).  Built once per process; every builder is deterministic."""
import functools

import numpy as np

import query_ref
import synth

CHUNK, PIECE = 16384, 64
WIDTH = 60                                                   # bases per line of the one-record texts


@functools.lru_cache(maxsize=None)
def one_record() -> bytes:
    """One gap-free record of 40 000 bases on 60-column lines: three 16 KiB chunks."""
    text = query_ref._record(b"one record", query_ref._bases(np.random.default_rng(900), 40_000))
    assert 2 * CHUNK < len(text) < 3 * CHUNK
    return text


def base_offset(head: int, b: int) -> int:
    """Text offset of base b of a record whose sequence begins at offset `head`, on 60-column lines."""
    return head + b + b // WIDTH


def base_at(head: int, off: int) -> int:
    """The base at text offset `off` (the one before it where `off` is a line terminator)."""
    q, r = divmod(off - head, WIDTH + 1)
    return q * WIDTH + min(r, WIDTH - 1)


GAP_HEAD = len(b">gaps\n")


@functools.lru_cache(maxsize=None)
def gapped(k: int = 5):
    """(text, runs): one record of A, C, G, T and N on 60-column lines, eleven 16 KiB chunks.  Runs of N of length 1, k-1,
    k, 63, 64, 65 and 300 lie inside a 64-byte piece (those that fit) or begin in the middle of one, lie across a piece seam
    and across the seams of the 16 KiB chunks 1 .. 7; one run covers chunk 9 whole (no valid base in it); the record begins
    with a run of 64 and ends with one of 65.  runs: (first base, length) of each, in text order."""
    head, n = GAP_HEAD, 175_000
    seq = bytearray(query_ref._bases(np.random.default_rng(901), n))
    lengths = (1, k - 1, k, 63, 64, 65, 300)
    runs = [(0, 64), (n - 65, 65)]
    for i, L in enumerate(lengths):
        # from byte 5 of a piece in chunk 0 (the short ones stay inside it), 700 bytes apart
        runs.append((base_at(head, 1024 + 704 * i + 5), L))
        # across a piece seam of chunk 0: the seam in the middle of the run (a run of 1: the last byte before the seam)
        runs.append((base_at(head, 8192 + 704 * i - (L + 1) // 2), L))
        # across the chunk seam i + 1, two thirds of the run before it
        runs.append((base_at(head, CHUNK * (i + 1) - max(1, 2 * L // 3)), L))
    runs.append((base_at(head, 9 * CHUNK - 100), base_at(head, 10 * CHUNK + 100) - base_at(head, 9 * CHUNK - 100)))
    runs.sort()
    for (a, la), (b, _) in zip(runs, runs[1:]):
        assert a + la + 2 * k < b, "runs too close"
    for lo, L in runs:
        seq[lo:lo + L] = b"N" * L
    text = query_ref._record(b"gaps", bytes(seq), WIDTH)
    assert 10 * CHUNK + 200 < len(text) < 11 * CHUNK
    body = np.frombuffer(text, dtype=np.uint8)
    chunk9 = body[9 * CHUNK:10 * CHUNK]
    assert not np.isin(chunk9, np.frombuffer(b"ACGT", dtype=np.uint8)).any()
    for i, L in enumerate(lengths):                          # what the placements promise
        at = CHUNK * (i + 1)
        assert body[at - 1] in b"N\n" and (L == 1 or body[at] in b"N\n" or body[at + 1] == ord("N"))
    return text, tuple(runs)


def _seq_line(rng, n: int) -> bytes:
    return query_ref._bases(rng, n) + b"\n"


@functools.lru_cache(maxsize=None)
def blanks() -> bytes:
    """Records with interior blanks and tabs, leading and trailing blanks, CRLF, lone CR and blank lines, text before the
    first header, and pending blanks that end a 64-byte piece and a 16 KiB chunk and then turn out interior (a base follows)
    or trailing (a terminator follows)."""
    rng = np.random.default_rng(902)
    parts = [b"  ACGTTGCAAC GT\nTTGACCA\n \n"]                 # before the first header: no record, no position

    def size():
        return sum(len(p) for p in parts)

    def pad_to(off: int):
        """one unwrapped sequence line that ends (with its terminator) at text offset `off`"""
        need = off - size()
        assert need >= 2, (off, size())
        parts.append(_seq_line(rng, need - 1))

    parts.append(b">r1 interior blanks and tabs\n")
    parts.append(b"ACGTTGCAAC GTACGGTCAT\tACGTTGACCA  \t ACGGTCATTG\n")
    parts.append(b"AC GT\nACGTTGCAAGGTCA\n")
    parts.append(b">r2 leading and trailing blanks, CRLF, lone CR, blank lines\n")
    parts.append(b"  \t ACGTTGCAAGGTACGT  \n\tTTGACCATGACGTA\t\r\nACGGTCATTGACCAGT\rTTGACGGTCATT\n\n\r\n   \n \t \r\nGGTCATTGACCA\n")
    parts.append(b">r3 pending blanks at the seams\n")
    # at a piece seam: three blanks end the piece, a base follows (interior); then the same with a terminator (trailing)
    pad_to(20 * PIECE - 13)
    parts.append(b"ACGTTGCAAC   " + b"GGTCATTGACCATG\n")
    assert (size() - 15) % PIECE == 0
    pad_to(40 * PIECE - 13)
    parts.append(b"ACGTTGCAAC   " + b"\nGGTCATTGACCATG\n")
    # blanks across a piece seam, two on either side, interior
    pad_to(60 * PIECE - 12)
    parts.append(b"ACGTTGCAAC  " + b"  GGTCATTGACCATG\n")
    # at the chunk seam: interior
    pad_to(CHUNK - 14)
    parts.append(b"ACGTTGCAAC \t  " + b"GGTCATTGACCATG \n")
    assert size() - 16 == CHUNK
    parts.append(b">r4\n")
    # at the next chunk seam: trailing (a CR follows), then a line that begins with blanks
    pad_to(2 * CHUNK - 13)
    parts.append(b"ACGTTGCAAC   " + b"\r   GGTCATTGACCATG\n")
    # blanks across the third chunk seam, interior, the line begun a piece earlier
    pad_to(3 * CHUNK - 80)
    parts.append(query_ref._bases(rng, 78) + b"  " + b" \tGGTCATTGACCATG\n")
    parts.append(b">r5 blanks only\n   \n\t\n>r6\nACGTTGCAAC GTACG\n")
    text = b"".join(parts)
    assert 3 * CHUNK < len(text) < 4 * CHUNK
    return text


@functools.lru_cache(maxsize=None)
def many_records(s: int) -> bytes:
    return query_ref.long_after_short(s, seed=900 + s, ragged=True, k=5)[0]


@functools.lru_cache(maxsize=None)
def short_reads() -> bytes:
    """5 000 reads of twelve bases: more records in one feed than a fresh indexer's record array holds."""
    rng = np.random.default_rng(903)
    return b"".join(b">r\n" + query_ref._bases(rng, 12) + b"\n" for _ in range(5000))


@functools.lru_cache(maxsize=None)
def fastq_reads() -> bytes:
    """300 reads of 1 .. 150 bases with Ns; quality lines that begin with '@' and '>'; CRLF in a third of the reads."""
    rng = np.random.default_rng(904)
    out = []
    for i in range(300):
        n = int(rng.integers(1, 151))
        seq = np.frombuffer(b"ACGTACGTACGTN", dtype=np.uint8)[rng.integers(0, 13, n)].tobytes()
        qual = bytearray(rng.integers(33, 74, n, dtype=np.uint8).tobytes())
        if i % 4 == 1:
            qual[0] = ord("@")
        elif i % 4 == 2:
            qual[0] = ord(">")
        nl = b"\r\n" if i % 3 == 0 else b"\n"
        out.append(b"@read%d extra" % i + nl + seq + nl + b"+" + nl + bytes(qual) + nl)
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def k17_genomes():
    return tuple(bytes(synth.family(i, 200_000)[0]) for i in range(2))


def k17_text() -> bytes:
    g = k17_genomes()
    return g[1] + g[0]                                       # another family member, then the indexed genome itself


def all_texts():
    """(name, text, k, fmt) of every text the GPU tests query."""
    return [("one_record_k5", one_record(), 5, "fasta"), ("one_record_k9", one_record(), 9, "fasta"),
            ("gapped_k5", gapped(5)[0], 5, "fasta"), ("gapped_k9", gapped(9)[0], 9, "fasta"),
            ("blanks", blanks(), 5, "fasta"), ("many_127", many_records(127), 5, "fasta"), ("many_200", many_records(200), 5, "fasta"),
            ("short_reads", short_reads(), 5, "fasta"), ("fastq", fastq_reads(), 9, "fastq"), ("k17", k17_text(), 17, "fasta")]
