"""The yardstick of the covered bases and of the masked text: the definition restated byte by byte on the host,
independently of the kernels.

A VALID BASE is a byte of ACGTacgt that is a sequence character of a record (text before the first header has none); the
valid bases of a text are numbered g = 0, 1, .. in text order.  A valid window is k consecutive positions that all hold valid
bases (query_coords_ref); its k-mer comes from oracle.kmer_list, which lists the windows in the same text order.  A window
MATCHES iff min <= T_t[a] <= max in at least one table; a valid base is COVERED iff it lies in a matching window.  The
selected bases are the covered ones, or with `invert` the valid bases that are not covered; the masked text is the input with
the selected bytes lower-cased (byte | 0x20), or with `hard` replaced by N, and masked[r] counts the selected bases of record r.
"""
from typing import Sequence

import numpy as np

import oracle
from query_coords_ref import BASES, BLANKS, TERMINATORS

_START, _HEADER, _SEQ = 0, 1, 2


def walk(fasta: bytes, k: int):
    """(base_off (B,) int64: the byte offset of every valid base; base_rec (B,) int64: its record; win_end (V,) int64: the
    ordinal g of the last base of every valid window, in text order; n_records).  The bases of a window are the ordinals
    g-k+1 .. g: `run` holds the byte offsets of the current run's bases, and its last k are the window's."""
    base_off, base_rec, win_end = [], [], []
    state, pending, rec = _START, 0, -1                      # rec = -1 before the first header
    run = []                                                 # byte offsets of the bases of the current run
    for off, c in enumerate(bytes(fasta)):
        if c in TERMINATORS:                                 # pending blanks were trailing
            state, pending = _START, 0
            continue
        if state == _HEADER:
            continue
        blank = c in BLANKS
        if state == _START:
            if blank:                                        # leading blanks
                continue
            if c == ord(">"):
                state, pending, rec, run = _HEADER, 0, rec + 1, []
                continue
            state = _SEQ
        if blank:
            pending += 1
            continue
        if pending:                                          # the blanks were interior: none is a base
            pending, run = 0, []
        if c not in BASES:
            run = []
            continue
        if rec < 0:                                          # text before the first header: no record, no valid base
            continue
        run.append(off)
        base_off.append(off)
        base_rec.append(rec)
        if len(run) >= k:
            g = len(base_off) - 1
            assert base_off[g - k + 1] == run[-k], "the bases of a window are not consecutive ordinals"
            win_end.append(g)
    return (np.array(base_off, dtype=np.int64), np.array(base_rec, dtype=np.int64), np.array(win_end, dtype=np.int64), rec + 1)


def walk_fast(fasta: bytes, k: int):
    """walk() in array operations, for texts too long for a byte loop (tests/test_mask_host.py holds the two equal on every
    other text): lines are cut at the terminators; a line whose first non-blank byte is '>' is a header line; every other
    non-blank byte is a sequence character; a run of valid bases is broken by a sequence character that is no base, by a
    header and by blanks with sequence characters on either side of them on their line."""
    b = np.frombuffer(bytes(fasta), dtype=np.uint8)
    n = b.size
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    term = np.isin(b, np.frombuffer(bytes(TERMINATORS), dtype=np.uint8))
    blank = np.isin(b, np.frombuffer(bytes(BLANKS), dtype=np.uint8))
    line = np.concatenate([[0], np.cumsum(term)[:-1]])       # a terminator belongs to the line it ends
    n_lines = int(line[-1]) + 1
    ink = ~blank                                             # (terminators are blanks)
    idx = np.arange(n)
    first = np.full(n_lines, n, dtype=np.int64)
    np.minimum.at(first, line[ink], idx[ink])
    last = np.full(n_lines, -1, dtype=np.int64)
    np.maximum.at(last, line[ink], idx[ink])
    has = first < n
    is_hdr_line = np.zeros(n_lines, dtype=bool)
    is_hdr_line[has] = b[first[has]] == ord(">")
    hdr_start = np.zeros(n, dtype=bool)
    hdr_start[first[is_hdr_line]] = True
    rec = np.cumsum(hdr_start) - 1                           # the record a byte lies in, -1 before the first header
    in_hdr = is_hdr_line[line]
    seqchar = ink & ~in_hdr
    is_base = np.isin(b, np.frombuffer(bytes(BASES), dtype=np.uint8))
    interior = blank & ~term & ~in_hdr & (idx > first[line]) & (idx < last[line])
    breaks = np.cumsum((seqchar & ~is_base) | hdr_start | interior)
    valid = seqchar & is_base & (rec >= 0)
    base_off = np.flatnonzero(valid).astype(np.int64)
    base_rec = rec[base_off].astype(np.int64)
    # a base continues the run of the one before iff no break lies between them and the one before it is valid too: a
    # base of dead text (before the first header) is no base, and there is none behind the first header
    brk = breaks[base_off]
    new_run = np.ones(base_off.size, dtype=bool)
    new_run[1:] = brk[1:] != brk[:-1]
    run_first = np.maximum.accumulate(np.where(new_run, np.arange(base_off.size), 0))
    in_run = np.arange(base_off.size) - run_first            # bases of the run before this one
    win_end = np.flatnonzero(in_run >= k - 1).astype(np.int64)
    return base_off, base_rec, win_end, int(rec[-1]) + 1


def expected(text: bytes, k: int, tables: Sequence, min_count: int = 1, max_count: int = 255, fast: bool = False) -> dict:
    """dict(valid (len(text),) bool, base_off, base_rec, n_bases, n_records, cover (n_bases,) bool, bits: cover packed as
    pk_query_cover packs it, win_end, match (V,) bool).  `tables`: u8 arrays of 4^k bytes or anything indexable by k-mers."""
    base_off, base_rec, win_end, n_records = (walk_fast if fast else walk)(text, k)
    kmers = oracle.kmer_list(text, k)
    assert kmers.size == win_end.size, "the walker and the oracle disagree on the valid windows"
    match = np.zeros(win_end.size, dtype=bool)
    for table in tables:
        c = np.asarray(table[kmers]).astype(np.int64)
        match |= (c >= min_count) & (c <= max_count)
    n_bases = base_off.size
    edge = np.zeros(n_bases + 1, dtype=np.int64)
    np.add.at(edge, win_end[match] - (k - 1), 1)
    np.add.at(edge, win_end[match] + 1, -1)
    cover = np.cumsum(edge)[:n_bases] > 0
    valid = np.zeros(len(text), dtype=bool)
    valid[base_off] = True
    return {"valid": valid, "base_off": base_off, "base_rec": base_rec, "n_bases": n_bases, "n_records": n_records, "cover": cover,
            "bits": pack(cover), "win_end": win_end, "match": match}


def pack(cover) -> np.ndarray:
    """One bit per base, bit g at byte g // 8, bit g % 8."""
    return np.packbits(np.asarray(cover, dtype=bool), bitorder="little")


def unpack(bits, n_bases: int) -> np.ndarray:
    return np.unpackbits(np.asarray(bits, dtype=np.uint8), bitorder="little")[:n_bases].astype(bool)


def selected(want: dict, invert: bool = False, cover=None) -> np.ndarray:
    """(n_bases,) bool: the covered bases, or with `invert` the valid bases that are not covered; `cover` stands in for the
    reference's own."""
    cover = want["cover"] if cover is None else np.asarray(cover, dtype=bool)
    return ~cover if invert else cover


def masked_text(text: bytes, want: dict, hard: bool = False, invert: bool = False, cover=None) -> bytes:
    out = np.frombuffer(bytes(text), dtype=np.uint8).copy()
    at = want["base_off"][selected(want, invert, cover)]
    out[at] = ord("N") if hard else out[at] | 0x20
    return out.tobytes()


def masked_counts(want: dict, invert: bool = False, cover=None) -> np.ndarray:
    """(R,) uint64: the selected bases of every record."""
    return np.bincount(want["base_rec"][selected(want, invert, cover)], minlength=want["n_records"]).astype(np.uint64)
