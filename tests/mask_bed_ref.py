"""The yardstick of the masked intervals (mask.py --bed): the definition restated byte by byte on the host, independently
of the kernels.

POSITIONS are those of query.py --coords, counted as seq_len counts them: within a record every sequence character gets the
next position (0-based), valid base or not; a blank inside a sequence line gets one once a non-blank sequence character
follows it on the same line; line terminators, leading and trailing blanks, header text and text before the first header get
none.  An INTERVAL is a maximal run of consecutive positions of one record that all hold selected bases: (record, start,
end), half-open.  Anything that holds a position and is not a selected base ends a run, and so do a header and the end of the
stream; what holds no position does not.
"""
import numpy as np

from query_coords_ref import BLANKS, TERMINATORS

_START, _HEADER, _SEQ = 0, 1, 2


def positions(text: bytes):
    """(rec (len(text),) int64, pos (len(text),) int64): per byte its record and position, or -1 and -1."""
    n = len(text)
    rec_of, pos_of = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    state, rec, pos = _START, -1, 0
    pending = []                                             # byte offsets of the blanks that no sequence character has followed yet
    for off, c in enumerate(bytes(text)):
        if c in TERMINATORS:                                 # pending blanks were trailing
            state, pending = _START, []
            continue
        if state == _HEADER:
            continue
        blank = c in BLANKS
        if state == _START:
            if blank:                                        # leading blanks
                continue
            if c == ord(">"):
                state, rec, pos, pending = _HEADER, rec + 1, 0, []
                continue
            state = _SEQ
        if blank:
            pending.append(off)
            continue
        for at in pending + [off]:                           # the blanks were interior: each holds a position
            if rec >= 0:
                rec_of[at], pos_of[at] = rec, pos
            pos += 1
        pending = []
    return rec_of, pos_of


def runs(rec, pos, keep):
    """The intervals of the positions (rec[i], pos[i]), given in stream order, that `keep` marks: a marked position goes on
    the run of the marked position before it iff it is the same record's next position."""
    rec, pos = np.asarray(rec, dtype=np.int64)[keep], np.asarray(pos, dtype=np.int64)[keep]
    if rec.size == 0:
        return tuple(np.zeros(0, dtype=np.uint64) for _ in range(3))
    new = np.ones(rec.size, dtype=bool)
    new[1:] = (rec[1:] != rec[:-1]) | (pos[1:] != pos[:-1] + 1)
    first = np.flatnonzero(new)
    last = np.concatenate([first[1:], [rec.size]]) - 1
    return rec[first].astype(np.uint64), pos[first].astype(np.uint64), (pos[last] + 1).astype(np.uint64)


def intervals(text: bytes, selected_bytes):
    """(iv_record, iv_start, iv_end), each (M,) uint64 in stream order, of the text whose selected bases are the bytes that
    `selected_bytes` ((len(text),) bool) marks."""
    rec, pos = positions(text)
    sel = np.asarray(selected_bytes, dtype=bool)
    assert sel.shape == (len(text),) and (pos[sel] >= 0).all(), "a selected byte holds no position"
    return runs(rec, pos, sel)


def intervals_one_plain_record(text: bytes, want: dict, selected_bases):
    """intervals() without a byte loop for a text that is one record in which every sequence character is a valid base
    (mask_inputs.long_text()): a base's position is its ordinal.  want: mask_ref.expected(text, ..); selected_bases: (n_bases,)."""
    body = np.frombuffer(bytes(text), dtype=np.uint8)
    head = bytes(text).index(b"\n")
    assert bytes(text)[:1] == b">" and want["n_records"] == 1 and b">" not in bytes(text)[1:]
    seq = body[head + 1:]
    plain = np.isin(seq, np.frombuffer(b"ACGTacgt\n", dtype=np.uint8))
    assert plain.all() and int((seq != 10).sum()) == want["n_bases"], "a sequence character that is no valid base"
    n = want["n_bases"]
    return runs(np.zeros(n, dtype=np.int64), np.arange(n, dtype=np.int64), np.asarray(selected_bases, dtype=bool))


def selected_bytes(text: bytes, want: dict, invert: bool = False, cover=None) -> np.ndarray:
    """(len(text),) bool from mask_ref.expected's result: the bytes of the selected bases."""
    import mask_ref
    out = np.zeros(len(text), dtype=bool)
    out[want["base_off"][mask_ref.selected(want, invert, cover)]] = True
    return out


def paint(text: bytes, iv_record, iv_start, iv_end) -> np.ndarray:
    """(len(text),) bool: the bytes whose (record, position) lies in one of the intervals."""
    rec, pos = positions(text)
    out = np.zeros(len(text), dtype=bool)
    if len(iv_record) == 0:
        return out
    span = np.int64(len(text) + 1)                           # more than any position: (record, position) as one ascending key
    lo = np.asarray(iv_record, dtype=np.int64) * span + np.asarray(iv_start, dtype=np.int64)
    hi = np.asarray(iv_record, dtype=np.int64) * span + np.asarray(iv_end, dtype=np.int64)
    assert (lo[1:] >= hi[:-1]).all() and (lo < hi).all(), "intervals out of order"
    held = np.flatnonzero(pos >= 0)
    key = rec[held] * span + pos[held]
    at = np.searchsorted(lo, key, side="right") - 1
    out[held] = (at >= 0) & (key < hi[np.maximum(at, 0)])
    return out


def bed_lines(chroms, iv_record, iv_start, iv_end) -> bytes:
    return "".join(f"{chroms[int(r)]}\t{int(a)}\t{int(b)}\n" for r, a, b in zip(iv_record, iv_start, iv_end)).encode("utf-8")
