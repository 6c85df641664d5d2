"""Plain-Python restatement of the base-quality rule (README "Base quality"), for the tests only.

mask_fastq_to_fasta(data, T) is the FASTA text a FASTQ stream stands for under the threshold byte T = Q + offset: byte i of
a record's line 2 becomes 'N' when byte i of its line 4 is below T (as an unsigned byte) and the line-2 byte is not one of
the str.strip() blanks.  Everything else is fastq_ref.fastq_to_fasta: the same bytes, the same length, the same errors.
"""
from typing import Tuple

import numpy as np

from fastq_ref import WS, fastq_to_fasta, lines


def mask_fastq_to_fasta(data: bytes, T: int) -> Tuple[bytes, int]:
    """(FASTA text, number of replaced bytes); T = 0 is off.  Raises FastqError exactly where fastq_to_fasta does."""
    assert 0 <= T <= 255
    data = bytes(data)
    plain = fastq_to_fasta(data)                             # the malformed-file rules, on the unmasked bytes
    ls = lines(data)
    out, n_masked = [], 0
    for r in range(0, len(ls), 4):
        (s1, e1, _), = ls[r:r + 1]
        if s1 == e1:                                         # blank lines after the last record
            break
        (s2, e2, t2), (s4, e4, _) = ls[r + 1], ls[r + 3]
        seq = bytearray(data[s2:e2])
        qual = data[s4:e4]
        assert len(qual) == len(seq)
        for i, q in enumerate(qual):
            if q < T and seq[i] not in WS:
                seq[i] = ord("N")
                n_masked += 1
        out.append(b">" + data[s1 + 1:s2] + bytes(seq) + data[e2:t2])
    fasta = b"".join(out)
    assert len(fasta) == len(plain)
    return fasta, n_masked


def with_qualities(fq: bytes, choose) -> bytes:
    """`fq` (well-formed) with every quality line replaced: choose(record index, length) -> that many bytes, none of them a
    line terminator.  Lengths, terminators and everything else stay."""
    fq = bytes(fq)
    ls = lines(fq)
    out, pos = [], 0
    for r in range(0, len(ls), 4):
        if ls[r][0] == ls[r][1] or r + 3 >= len(ls):
            break
        s4, e4, _ = ls[r + 3]
        q = bytes(choose(r // 4, e4 - s4))
        assert len(q) == e4 - s4 and b"\n" not in q and b"\r" not in q
        out.append(fq[pos:s4] + q)
        pos = e4
    out.append(fq[pos:])
    return b"".join(out)


def biased_qualities(fq: bytes, T: int, share: float, seed: int) -> bytes:
    """Quality bytes T + 0 .. 9 with about `share` of them in T - 10 .. T - 1 (no line terminators: 10 and 13 are stepped over)."""
    rng = np.random.default_rng(seed)

    def choose(_, n):
        q = T + rng.integers(0, 10, n)
        low = rng.random(n) < share
        q[low] = T - 1 - rng.integers(0, 10, int(low.sum()))
        q = np.clip(q, 1, 255)
        q[(q == 10) | (q == 13)] = 11 if T > 11 else 14
        return q.astype(np.uint8).tobytes()
    return with_qualities(fq, choose)


def hand_qualities(fq: bytes, T: int, seed: int) -> bytes:
    """Quality bytes drawn from {T - 1, T, T + 1, 0x00, 0xFF, '@', '+', '>'} (those in 0 .. 255 that are no terminators)."""
    pool = [b for b in (T - 1, T, T + 1, 0x00, 0xFF, ord("@"), ord("+"), ord(">")) if 0 <= b <= 255 and b not in (10, 13)]
    rng = np.random.default_rng(seed)
    return with_qualities(fq, lambda r, n: bytes(pool[int(j)] for j in rng.integers(0, len(pool), n)))
