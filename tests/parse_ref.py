"""oracle/pyoracle.py's records() / windows() restated on `bytes`, with no decode -- for the tests only.

pyoracle decodes its input as UTF-8 first, so it cannot say what a byte >= 0x80 means.  The project's rule (DESIGN.md 2,
"Domain limits of the parser") is stated on bytes: lines end at \\n, \\r and \\r\\n; a line is stripped of the ten ASCII
blanks str.strip() knows; a line whose first remaining byte is '>' opens a record; every other byte of a sequence line is one
sequence character, and only ACGTacgt map to a base.  This module is that rule, read side by side with pyoracle.records.
"""
import re

import numpy as np

WS = b" \t\n\v\f\r\x1c\x1d\x1e\x1f"                       # what str.strip() strips, ASCII only
_LINE_END = re.compile(rb"\r\n|\r|\n")

NONE = 4                                                   # pyoracle's None
CONV = np.full(256, NONE, dtype=np.uint8)                  # only ACGTacgt map to a base; bytes >= 0x80 are NONE like any other
for _v, _c in enumerate(b"ACGT"):
    CONV[_c] = _v
    CONV[_c | 0x20] = _v

RECORD_DTYPE = np.dtype([("name_off", "<u8"), ("name_len", "<u8"), ("seq_len", "<u8"), ("n_valid_kmers", "<u8")])


def lines(data: bytes):
    """(offset, raw line) for every line of the stream, terminators removed."""
    pos = 0
    for m in _LINE_END.finditer(data):
        yield pos, data[pos:m.start()]
        pos = m.end()
    yield pos, data[pos:]


def records(data: bytes):
    """pyoracle.records on bytes: (name_off, name_len, sequence bytes) per record; name_off is the byte behind the '>'."""
    name = None
    parts = []
    for off, raw in lines(bytes(data)):
        line = raw.strip(WS)
        if not line:
            continue
        if line[0] == ord(">"):
            if name is not None:
                yield name[0], name[1], b"".join(parts)
            lead = len(raw) - len(raw.lstrip(WS))
            name = (off + lead + 1, len(line) - 1)
            parts = []                                     # also drops lines seen before the first header
        else:
            parts.append(line)
    if name is not None:
        yield name[0], name[1], b"".join(parts)


def windows(seq: bytes, k: int) -> np.ndarray:
    """pyoracle.windows on bytes: the canonical value min(fwd, rev) of every None-free window, in text order (u64)."""
    codes = CONV[np.frombuffer(seq, dtype=np.uint8)].astype(np.uint64)
    if codes.size < k:
        return np.zeros(0, dtype=np.uint64)
    win = np.lib.stride_tricks.sliding_window_view(codes, k)
    ok = (win != NONE).all(axis=1)
    win = win[ok]
    weight = np.array([4 ** (k - p - 1) for p in range(k)], dtype=np.uint64)
    fwd = (win * weight).sum(axis=1, dtype=np.uint64)
    rev = ((np.uint64(3) - win) * weight[::-1]).sum(axis=1, dtype=np.uint64)
    return np.minimum(fwd, rev)


def parse(data: bytes, k: int):
    """(records[RECORD_DTYPE], canonical k-mers of all records in text order)."""
    recs, kmers = [], []
    for name_off, name_len, seq in records(data):
        w = windows(seq, k)
        recs.append((name_off, name_len, len(seq), w.size))
        kmers.append(w)
    return (np.array(recs, dtype=RECORD_DTYPE),
            np.concatenate(kmers) if kmers else np.zeros(0, dtype=np.uint64))


def names(data: bytes, recs) -> list:
    return [bytes(data[int(r["name_off"]):int(r["name_off"]) + int(r["name_len"])]) for r in recs]
