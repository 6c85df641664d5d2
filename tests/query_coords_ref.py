"""The yardstick of the base coordinates of binned query hits: the definition restated byte by byte on the host,
independently of the kernels and of oracle/.

Positions are counted within a record as seq_len counts them: every sequence character gets the next position (0-based),
valid base or not; blanks inside a sequence line count once a non-blank sequence character follows them on the same line;
line terminators, the leading and trailing blanks of a line, header text and text before the first header get none.  A valid
window is k consecutive positions that all hold one of ACGTacgt.  For the row of record r and bin b (bins of W valid
windows, query_bins_ref): bin_start = the position of the first base of window b*W, bin_end = one past the position of the
last base of window min((b+1)*W, m) - 1."""
from typing import Sequence

import numpy as np

import query_bins_ref
from fastq_ref import fastq_to_fasta

TERMINATORS = frozenset(b"\n\r")
BLANKS = frozenset(b"\t\n\v\f\r\x1c\x1d\x1e\x1f ")          # what str.strip() strips, ASCII
BASES = frozenset(b"ACGTacgt")
_START, _HEADER, _SEQ = 0, 1, 2


def walk(fasta: bytes, k: int):
    """Per record, in file order: (seq_len, [start position of every valid window, in text order])."""
    records = []
    state, pos, pending, run, starts = _START, 0, 0, 0, None     # starts is None before the first header
    for c in bytes(fasta):
        if c in TERMINATORS:                                 # pending blanks were trailing: they get no position
            state, pending = _START, 0
            continue
        if state == _HEADER:
            continue
        blank = c in BLANKS
        if state == _START:
            if blank:                                        # leading blanks
                continue
            if c == ord(">"):
                if starts is not None:
                    records.append((seq_len, starts))
                state, pos, pending, run, starts, seq_len = _HEADER, 0, 0, 0, [], 0
                continue
            state = _SEQ
        if blank:
            pending += 1
            continue
        if pending:                                          # the blanks were interior: each holds a position, none is a base
            pos, pending, run = pos + pending, 0, 0
        run = run + 1 if c in BASES else 0
        if run >= k and starts is not None:
            starts.append(pos - k + 1)
        pos += 1
        if starts is not None:
            seq_len = pos
    if starts is not None:
        records.append((seq_len, starts))
    return records


def window_starts(text: bytes, k: int, fmt: str = "fasta"):
    """(seq_len (R,), n_windows (R,), starts: the window start positions of all records, concatenated in text order)."""
    records = walk(fastq_to_fasta(text) if fmt == "fastq" else text, k)
    seq_len = np.array([r[0] for r in records], dtype=np.uint64)
    n_windows = np.array([len(r[1]) for r in records], dtype=np.uint64)
    starts = np.array([s for r in records for s in r[1]], dtype=np.uint64)
    return seq_len, n_windows, starts


def bin_coords(n_windows: np.ndarray, starts: np.ndarray, k: int, W: int):
    """(bin_start (B,), bin_end (B,)) uint64 of the rows query_bins_ref.bin_bounds lays out."""
    _, lo, hi, _, _ = query_bins_ref.bin_bounds(n_windows, W)
    return starts[lo].astype(np.uint64), (starts[hi - 1] + np.uint64(k)).astype(np.uint64)


def expected(text: bytes, k: int, tables: Sequence, min_count: int, max_count: int, W: int, fmt: str = "fasta") -> dict:
    """query_bins_ref.expected plus bin_start, bin_end (B,) uint64 and window_start (all windows, text order)."""
    out = query_bins_ref.expected(text, k, tables, min_count, max_count, W, fmt)
    seq_len, n_windows, starts = window_starts(text, k, fmt)
    assert np.array_equal(seq_len, out["seq_len"]) and np.array_equal(n_windows, out["n_valid"]), "the two walkers disagree"
    out["bin_start"], out["bin_end"] = bin_coords(n_windows, starts, k, W)
    out["window_start"] = starts
    return out


def check_consequences(want: dict, k: int, W: int, gap_free: bool = False) -> None:
    """What follows from the definition, for any result with bin_start / bin_end (the reference's or the GPU's)."""
    start, end = want["bin_start"].astype(np.int64), want["bin_end"].astype(np.int64)
    rec, n_win = want["row_record"], want["row_windows"].astype(np.int64)
    assert start.shape == end.shape == rec.shape
    assert np.all(0 <= start) and np.all(start < end) and np.all(end <= want["seq_len"].astype(np.int64)[rec])
    assert np.all(end - start >= n_win + k - 1)
    same = rec[1:] == rec[:-1]
    assert np.all(start[1:][same] > start[:-1][same])        # strictly increasing within a record
    if gap_free:
        b, m = want["row_bin"], want["n_valid"].astype(np.int64)[rec]
        Wc = min(int(W), 1 << 40)
        assert np.array_equal(start, b * Wc) and np.array_equal(end, np.minimum((b + 1) * Wc, m) + k - 1)
        assert np.array_equal(end - start, n_win + k - 1)
