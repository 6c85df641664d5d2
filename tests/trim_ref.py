"""The yardstick of trim.py (README "Trimming reads"): the definitions restated in plain Python on the references that exist,
independently of the kernels.

The FASTQ stands for a FASTA text (fastq_ref.fastq_to_fasta; with a quality threshold fastq_qual_ref.mask_fastq_to_fasta, which
turns the bases below it into N).  Positions are mask_bed_ref.positions of that text, valid and covered bases mask_ref's, and
a RUN is one of mask_bed_ref.intervals of the covered bases.  The KEPT RUN of a read is its longest run, among equals the one
with the smallest start; (0, 0) without a covered base.  trimmed_bytes writes a kept read straight from the definition of a
written record, not through segments, so that trim.trim_segments + filter_ref.select_bytes can be held against it.
"""
import numpy as np

import mask_bed_ref
import mask_ref
from fastq_qual_ref import mask_fastq_to_fasta
from fastq_ref import WS, lines

FIELDS = ("pos2", "pos4", "end2", "end4", "seq_len", "trim_start", "trim_end", "covered", "lead")


def record_lines(fq: bytes):
    """[(line 1, line 2, line 3, line 4, end of the record)] per record, each line (start, end of text, end of terminator); the
    blank lines behind the last record belong to it."""
    ls = lines(bytes(fq))
    groups = []
    for r in range(0, len(ls), 4):
        if ls[r][0] == ls[r][1]:                             # an empty line 1: only blank lines follow
            break
        groups.append(ls[r:r + 4])
    return [tuple(g) + (groups[i + 1][0][0] if i + 1 < len(groups) else len(fq),) for i, g in enumerate(groups)]


def starts(fq: bytes) -> np.ndarray:
    """(R + 1,) uint64: where every record begins, and the length of the stream."""
    return np.array([g[0][0] for g in record_lines(fq)] + [len(fq)], dtype=np.uint64)


def fasta_of(fq: bytes, T: int = 0) -> bytes:
    return mask_fastq_to_fasta(bytes(fq), T)[0]


def runs(fq: bytes, cover, k: int = None, min_count: int = 1, max_count: int = 255, T: int = 0, fast: bool = False) -> dict:
    """The nine FIELDS of every record, (R,) uint64 each, and n_bases, cover (n_bases,) bool and n_valid_bases (R,).
    `cover`: (n_bases,) bools, one per valid base of the stream in stream order, or a list of tables (then `k` and the count
    window say which windows match, and every run is asserted to be at least k long)."""
    fq = bytes(fq)
    fasta = fasta_of(fq, T)
    from_tables = not (isinstance(cover, np.ndarray) and cover.ndim == 1 and cover.dtype == bool)
    if from_tables:
        want = mask_ref.expected(fasta, k, cover, min_count, max_count, fast=fast)
        base_off, base_rec, cov = want["base_off"], want["base_rec"], want["cover"]
    else:
        base_off, base_rec, _, _ = (mask_ref.walk_fast if fast else mask_ref.walk)(fasta, 1)
        cov = cover
    assert cov.shape == base_off.shape, "one cover bit per valid base"
    recs = record_lines(fq)
    R = len(recs)
    rec_of, pos_of = mask_bed_ref.positions(fasta)
    selected = np.zeros(len(fasta), dtype=bool)
    selected[base_off[cov]] = True
    iv_record, iv_start, iv_end = mask_bed_ref.intervals(fasta, selected)
    out = {name: np.zeros(R, dtype=np.uint64) for name in FIELDS}
    best = [(0, 0)] * R
    for r, a, b in zip(iv_record.tolist(), iv_start.tolist(), iv_end.tolist()):    # stream order: ascending starts within a record
        assert b > a and (not from_tables or b - a >= k), "a non-empty run is at least k long: a covered base lies in a matching window"
        if b - a > best[r][1] - best[r][0]:
            best[r] = (a, b)
    held = pos_of >= 0
    seq_len = np.zeros(R, dtype=np.int64)
    np.maximum.at(seq_len, rec_of[held], pos_of[held] + 1)
    for r, (l1, l2, l3, l4, end) in enumerate(recs):
        line2 = fq[l2[0]:l2[1]]
        lead = len(line2) - len(line2.lstrip(WS))
        assert seq_len[r] == len(line2.strip(WS)) and l4[1] - l4[0] == len(line2)
        out["lead"][r], out["pos2"][r], out["pos4"][r] = lead, l2[0] + lead, l4[0] + lead
        out["end2"][r], out["end4"][r], out["seq_len"][r] = l2[1], l4[1], seq_len[r]
        out["trim_start"][r], out["trim_end"][r] = best[r]
        assert 0 <= best[r][0] <= best[r][1] <= seq_len[r]
    out["covered"] = np.bincount(base_rec[cov], minlength=R).astype(np.uint64)
    out.update(n_bases=int(base_off.size), cover=np.asarray(cov, dtype=bool), n_valid_bases=np.bincount(base_rec, minlength=R).astype(np.uint64))
    return out


def keep_of(want: dict, min_len: int) -> np.ndarray:
    return ((want["trim_end"] - want["trim_start"]).astype(np.int64) >= min_len).astype(np.uint8)


def classes(want: dict, min_len: int):
    """The shares of the reads that stay whole, are cut, and are dropped at `min_len`."""
    length = (want["trim_end"] - want["trim_start"]).astype(np.int64)
    kept = length >= min_len
    whole = kept & (length == want["seq_len"].astype(np.int64))
    n = max(1, kept.size)
    return whole.sum() / n, (kept & ~whole).sum() / n, (~kept).sum() / n


def trimmed_bytes(fq: bytes, trim_start, trim_end, keep) -> bytes:
    """The trimmed file: per kept read line 1 with its terminator, the bytes of line 2 that hold the positions [start, end),
    line 2's terminator, line 3 with its terminator, the bytes of line 4 at the same offsets, and everything of the record
    behind line 4's content."""
    fq = bytes(fq)
    out = []
    for r, (l1, l2, l3, l4, end) in enumerate(record_lines(fq)):
        if not keep[r]:
            continue
        line2 = fq[l2[0]:l2[1]]
        lead = len(line2) - len(line2.lstrip(WS))
        a, b = lead + int(trim_start[r]), lead + int(trim_end[r])
        out += [fq[l1[0]:l1[2]], line2[a:b], fq[l2[1]:l2[2]], fq[l3[0]:l3[2]], fq[l4[0]:l4[1]][a:b], fq[l4[1]:end]]
    return b"".join(out)


def rest_bytes(fq: bytes, keep) -> bytes:
    """The records that were not kept, as their own bytes."""
    fq = bytes(fq)
    return b"".join(fq[l1[0]:end] for r, (l1, _, _, _, end) in enumerate(record_lines(fq)) if not keep[r])
