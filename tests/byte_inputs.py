"""Seeded FASTA / FASTQ texts over all 256 byte values, one generator per route a byte can take through the parser
kernels (fasta_fsm.h piece_scan sparse / dense, the squeeze pass's header and byte-wise routes, fastq.hip fq_masks).

No route counter is exposed by the library, so every generator asserts on the host, with numpy, the condition that
sends its text down the route it is meant for; a later change here cannot silently stop exercising that route.
Every text stays under 1 MB.
"""
import functools

import numpy as np

import oracle
from parse_ref import WS

PIECE = 64                                   # bytes one lane walks (fasta_fsm.h)
WAVE = 64 * PIECE                            # one wavefront: 64 consecutive pieces, 4 KiB aligned
CHUNK = 256 * PIECE                          # one workgroup: 16 KiB
SPARSE_MAX = 6                               # piece_scan: the wave goes four bytes at a time once a piece has more non-bases
WIDTH = 61                                   # bases per line of the placement texts
BASES = np.frombuffer(b"ACGTacgt", dtype=np.uint8)
BLANKS = bytes(c for c in WS if c not in b"\r\n")          # the eight blanks that end no line
PIECE_OFFSETS = (0, 1, 31, 62, 63)
SEAM_SIDES = ((-2, 1), (-1, 0), (-2, 0), (-1, 1))          # (left, right) of a seam: two values share one seam
NEAR_MISSES_OF_GT = (0xBE, 0x1E, 0x3C, 0x3F, 0x7E)         # '>' with one bit flipped: none of them opens a record

_IS_BASE = np.zeros(256, dtype=bool)
_IS_BASE[BASES] = True


def non_bases_per_piece(text: bytes) -> np.ndarray:
    """Number of bytes outside ACGTacgt (line terminators included) in every 64-byte piece of the text."""
    a = np.frombuffer(text, dtype=np.uint8)
    pad = np.ones(-a.size % PIECE, dtype=np.uint8) * ord("A")
    return (~_IS_BASE[np.concatenate([a, pad])]).reshape(-1, PIECE).sum(axis=1)


def _rand_bases(rng, n: int) -> np.ndarray:
    return BASES[rng.choice(8, size=n, p=[0.2, 0.2, 0.2, 0.2, 0.05, 0.05, 0.05, 0.05])]


def _base4_name(b: int, n: int = 4) -> bytes:
    """The value written in base letters: header text that adds no non-base to its piece."""
    return bytes(b"ACGT"[(b >> (2 * i)) & 3] for i in reversed(range(n)))


# ------------------------------------------------------------------ placement_fasta --------------------------------------
def _placement_text(values, dense: bool, seed: int):
    """One text for `values`: a canvas of 61-base lines; per value one record (a header line of base letters) with the
    value at piece offsets 0, 1, 31, 62, 63, and two values on either side of every 16 KiB seam.  Returns
    (text, offsets of every placement)."""
    rng = np.random.default_rng(seed)
    values = list(values)
    n_seams = (len(values) + 1) // 2
    n_lines = ((n_seams + 1) * CHUNK - 700) // (WIDTH + 1)
    canvas = np.empty((n_lines, WIDTH + 1), dtype=np.uint8)
    canvas[:, :WIDTH] = _rand_bases(rng, n_lines * WIDTH).reshape(n_lines, WIDTH)
    canvas[:, WIDTH] = 10
    canvas = canvas.reshape(-1)[:-7].copy()                 # the text ends inside a line, in a partly filled piece
    placed = []

    def put(at: int, b: int):
        placed.append(at)
        if not dense:
            canvas[at] = b
            return
        run = int(rng.integers(3, 13))                      # b inside a run of 3-12 copies of itself, then Ns
        canvas[at:at + run] = b
        lo = at // PIECE * PIECE
        piece = canvas[lo:lo + PIECE]
        order = sorted((i for i in range(PIECE) if not at <= lo + i < at + run), key=lambda i: abs(lo + i - at))
        for i in order:
            if int((~_IS_BASE[piece]).sum()) > SPARSE_MAX:
                break
            if _IS_BASE[piece[i]]:
                piece[i] = ord("N")

    lines_per_value = n_lines // len(values)
    assert lines_per_value >= 14
    for i, b in enumerate(values):
        line = i * lines_per_value
        start = line * (WIDTH + 1)
        span = 14 * (WIDTH + 1)                              # header line and the five placements
        while -(-(start - 2 * PIECE) // CHUNK) * CHUNK < start + span + 2 * PIECE:   # keep them clear of the seams
            line += 1
            start = line * (WIDTH + 1)
        canvas[start:start + WIDTH] = np.frombuffer(b">" + _base4_name(b, WIDTH - 1), dtype=np.uint8)
        at = (start + 2 * (WIDTH + 1) + PIECE - 1) // PIECE * PIECE
        for off in PIECE_OFFSETS:                            # each in a piece of its own, two pieces apart
            put(at + off, b)
            at += 2 * PIECE
    for s in range(n_seams):
        seam = (s + 1) * CHUNK
        left, right = SEAM_SIDES[s % len(SEAM_SIDES)]
        pair = values[2 * s:2 * s + 2]
        put(seam + left, pair[0])                            # dense: the right run overwrites what the left one put behind the seam
        put(seam + right, pair[-1])
    return canvas.tobytes(), np.array(placed, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def placement_fasta(dense: bool):
    """Every byte value inside random ACGT text (lower case mixed in) wrapped at 61 columns: one record per value with the
    value at piece offsets 0, 1, 31, 62 and 63, and every value within two bytes of a 16 KiB chunk seam -- on ONE side of
    one seam per value (two values share a seam, the first at -2 or -1, the second at 0 or +1, so that each has bases on
    its far side; both sides for every value would take 256 seams).  256 values need 128 seams, 2 MB of text: the values
    are dealt over three texts of 44 chunks each.  dense: the run of the value on the left of a seam is cut off by the run
    on its right, so it keeps the 2 or 1 bytes in front of the seam (asserted below: the byte at every placement offset
    is the value, and its piece is over the threshold).  Values 10, 13 and 62 change the line structure where they land;
    the oracle decides what the text then means.

    dense=False: no 64-byte piece anywhere holds more than 6 non-bases, so every wave of piece_scan goes byte by byte.
    dense=True: every placement is a run of 3-12 copies of the value with Ns around it, >= 7 non-bases in its piece, so
    its wave goes four bytes at a time."""
    texts = []
    for g in range(3):
        values = list(range(g, 256, 3))
        text, placed = _placement_text(values, dense, seed=900 + 10 * g + dense)
        assert len(text) < 1_000_000
        per_piece = non_bases_per_piece(text)
        a = np.frombuffer(text, dtype=np.uint8)
        if dense:
            assert (per_piece[placed // PIECE] > SPARSE_MAX).all(), "a placement left the four-at-a-time route"
        else:
            # per 4 KiB-aligned block: no piece above the threshold (a wave is dense as soon as one piece is)
            blocks = np.concatenate([per_piece, np.zeros(-per_piece.size % 64, dtype=per_piece.dtype)]).reshape(-1, 64)
            assert (blocks.max(axis=1) <= SPARSE_MAX).all(), "a wave left the byte-by-byte route"
        for b in values:                                     # every value at every piece offset and next to a seam
            at = placed[a[placed] == b]
            assert set(PIECE_OFFSETS) <= set((at % PIECE).tolist()), b
            d = at % CHUNK
            assert ((d <= 1) | (d >= CHUNK - 2)).any(), b
        texts.append(text)
    return tuple(texts)


# ------------------------------------------------------------------ line starts -------------------------------------------
@functools.lru_cache(maxsize=None)
def line_start_fasta() -> bytes:
    """Every value as the first byte of a line: behind \\n, behind \\r\\n, and behind 1-3 leading blanks.  Only '>' may open
    a record there -- not 0xBE, 0x1E, 0x3C, 0x3F or 0x7E."""
    rng = np.random.default_rng(910)

    def seq(n):
        return _rand_bases(rng, n).tobytes()

    parts = [b">line starts\n" + seq(50) + b"\n"]
    for b in range(256):
        one = bytes([b])
        lead = bytes(BLANKS[int(i)] for i in rng.integers(0, len(BLANKS), size=1 + b % 3))
        parts.append(b">v%03d\n" % b + seq(30) + b"\n" + one + seq(20) + b"\n" + seq(25) + b"\r\n" + one + seq(20) + b"\r\n"
                     + seq(11) + b"\n" + lead + one + seq(20) + b"\n" + seq(17) + b"\n")
    text = b"".join(parts)
    a = np.frombuffer(text, dtype=np.uint8)
    after_nl = a[1:][a[:-1] == 10]
    assert np.unique(after_nl).size == 256                   # every value directly behind a \n (and behind \r\n)
    assert len(text) < 1_000_000
    return text


# what the first byte of a stream can be, by class: blanks, terminators, '>', its near misses, bases, the same with bit 7 set
STREAM_START_VALUES = tuple(sorted(set(WS) | set(NEAR_MISSES_OF_GT) | set(b">ACgtN@+;0") |
                                   {0x00, 0x01, 0x08, 0x0E, 0x1B, 0x21, 0x7F, 0x80, 0x85, 0x8A, 0x8D, 0xA0, 0xC1, 0xE7, 0xFF}))


def stream_start_fastas():
    """Short texts whose very first byte is the given value, one per class of value (STREAM_START_VALUES): the first line of
    a stream has no terminator in front of it."""
    assert len(STREAM_START_VALUES) <= 40
    rng = np.random.default_rng(911)
    return [bytes([b]) + _rand_bases(rng, 9).tobytes() + b"\n" + _rand_bases(rng, 12).tobytes() + b"\n>r\n" +
            _rand_bases(rng, 40).tobytes() + b"\n" for b in STREAM_START_VALUES]


# ------------------------------------------------------------------ header text -------------------------------------------
CLI_NAME_VALUES = (0x00, 0x1C, 0x20, 0x3E, 0x5C, 0x7F, 0x80, 0x85, 0xA0, 0xC2, 0xC3, 0xE2, 0xF0, 0xFF)
KEPT_AT_NAME_END = (0x80, 0x85, 0xA0, 0xFF, 0x7F)


def header_bytes_fasta(values=None) -> bytes:
    """Records whose names hold every value except 10 and 13 (or the given ones) at the start, in the middle and at the end
    of the name; names of 70 and 130 bytes (header text across pieces), and one name across a 16 KiB seam.  Trailing
    0x1C-0x1F, space and tab are stripped from a name, trailing 0x80, 0x85, 0xA0, 0xFF and 0x7F are kept: both asserted
    here from the oracle's records."""
    rng = np.random.default_rng(920)
    values = [b for b in (range(256) if values is None else values) if b not in (10, 13)]
    parts, size, seam_done = [], 0, False
    ends = {}

    def add(name: bytes, eol: bytes = b"\n"):
        nonlocal size
        rec = b">" + name + eol + _rand_bases(rng, int(rng.integers(8, 40))).tobytes() + eol
        parts.append(rec)
        size += len(rec)

    for b in values:
        one = bytes([b])
        if not seam_done and size > CHUNK - 1500:            # the name across the chunk seam: pad up to 40 bytes before it
            fill = _rand_bases(rng, CHUNK - 40 - size - 4).tobytes()
            parts.append(b">f\n" + fill + b"\n")
            size += len(fill) + 4
            assert size == CHUNK - 40
            add(b"across the seam " + one * 3 + b" " + bytes(range(0x7E, 0x7E + 60)))
            seam_done = True
        add(one + b"starts %d" % b)
        add(b"mid" + one + b"dle", b"\r\n" if b % 5 == 0 else b"\n")
        ends[b] = len(parts)
        add(b"ends" + one)
        if b % 16 == 5 or b in KEPT_AT_NAME_END:
            add((one + b"seventy ").ljust(69, b"x") + one)
            add((b"a hundred and thirty " + one + b" ").ljust(128, b"\xa0") + one + one)
    text = b"".join(parts)
    assert len(text) < 1_000_000 and (values != [b for b in range(256) if b not in (10, 13)] or seam_done)
    recs = oracle.count_fasta(text, 5)["records"]
    rec_at = {int(r["name_off"]) - 1: r for r in recs}
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    for b, i in ends.items():                                # the record ">ends" + b: is b part of the name?
        r = rec_at[int(off[i])]
        stripped = bytes([b]) in WS
        assert int(r["name_len"]) == (4 if stripped else 5), (b, int(r["name_len"]))
    for b in KEPT_AT_NAME_END:
        assert b not in ends or int(rec_at[int(off[ends[b]])]["name_len"]) == 5
    return text


# ------------------------------------------------------------------ soup -------------------------------------------------
@functools.lru_cache(maxsize=None)
def soup(seed: int, n: int, k_min: int = 3) -> bytes:
    """n random bytes over all 256 values; bases, \\n and '>' dominate.  Asserts that >= 200 distinct values occur and that
    the oracle finds >= 1000 valid k-mers at k_min (a soup with no windows proves nothing)."""
    rng = np.random.default_rng(seed)
    w = rng.random(256) ** 6 + 0.02                          # the floor: every value a few times in 10 000 bytes
    w[BASES] += 9.0
    w[10] += 3.0
    w[13] += 0.7
    w[32] += 0.7
    w[62] += 0.5
    data = rng.choice(256, size=n, p=w / w.sum()).astype(np.uint8).tobytes()
    data = b">" + data[1:]                                   # nothing in front of the first record
    assert np.unique(np.frombuffer(data, dtype=np.uint8)).size >= 200, "the soup misses too many values"
    assert oracle.kmer_list(data, k_min).size >= 1000, "the soup has too few windows"
    return data


SOUP_CASES = ((31, 69_999), (32, 65_537), (33, 49_153), (34, 32_768), (35, 16_385), (36, 12_001))   # (seed, length)
SOUP_PREFIXES = (1, 2, 3, 63, 64, 65, 4095, 4097)            # and the first bytes of the first soup: lengths from 1 up


def cuts_around_odd_bytes(data: bytes, seed: int, n: int = 60):
    """Feed boundaries immediately before and behind bytes >= 0x80 and bytes < 0x21 (so each of them is also a one-byte
    feed), for n such bytes picked at random, half of each kind."""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(data, dtype=np.uint8)
    high, low = np.flatnonzero(a >= 0x80), np.flatnonzero(a < 0x21)
    assert high.size >= n // 2 and low.size >= n // 2
    pick = np.concatenate([rng.choice(high, n // 2, replace=False), rng.choice(low, n // 2, replace=False)])
    cuts = np.unique(np.concatenate([[0, len(data)], pick, pick + 1]))
    return [int(c) for c in cuts if c <= len(data)]


# ------------------------------------------------------------------ FASTQ -------------------------------------------------
@functools.lru_cache(maxsize=None)
def placement_fastq(crlf: bool) -> bytes:
    """Well-formed four-line records with every value except 10 and 13 in every line role: in the name of line 1, in the
    text behind the '+' of line 3, in the qualities of line 4 (as long as line 2), and in the sequence of line 2 -- first
    byte of the line, inside, last byte, behind leading blanks and in front of trailing ones (the FASTQ front end keeps
    those bytes, the FASTA rules strip them), and directly in front of a '>' (rule 2 looks at the first non-blank byte
    of line 2 only)."""
    rng = np.random.default_rng(930 + crlf)
    nl = b"\r\n" if crlf else b"\n"
    out = []

    def seq(n):
        return _rand_bases(rng, n).tobytes()

    def rec(name: bytes, line2: bytes, plus: bytes = b"", qual: bytes = None):
        if qual is None:
            qual = bytes(rng.integers(33, 74, len(line2), dtype=np.uint8))
        assert len(qual) == len(line2) and not line2.lstrip(WS).startswith(b">")
        assert not any(c in b"\r\n" for c in name + line2 + plus + qual)
        out.append(b"@" + name + nl + line2 + nl + b"+" + plus + nl + qual + nl)

    for b in range(256):
        if b in (10, 13):
            continue
        one = bytes([b])
        blank = one in [bytes([c]) for c in WS]
        rec(one + b"name" + one + b" x" + one, seq(24))                                        # line 1
        rec(b"p%d" % b, seq(20), plus=one + b"again" + one)                                    # line 3
        rec(b"q%d" % b, seq(21), qual=one + b"IIIIIIIII" + one + b"FFFFFFFFF" + one)           # line 4
        inner = seq(9) + one + seq(9) + one
        rec(b"s%d" % b, (seq(3) if b == 62 else one) + inner)                                  # line 2: first, inside, last
        rec(b"b%d" % b, b" \t" + (seq(2) if b == 62 else one) + inner + b" \x1f")              # ... with blanks around
        if not blank and b != 62:
            rec(b"g%d" % b, one + b">" + seq(15))                                              # b, not '>', is the first non-blank
    text = b"".join(out)
    assert len(text) < 1_000_000
    return text


WALKER_AT = (10, 63, 64, 130)                # positions of a read: inside step 0, on either side of the first step seam, in step 2
WALKER_LEN = 200


@functools.lru_cache(maxsize=None)
def walker_fastq(genome: bytes = None) -> bytes:
    """Reads of 200 positions for the record walkers (kmer_trim.hip, kmer_correct.hip), whose steps are 64 positions: per
    value except 10 and 13 one read with the value at positions 10 and 64 of line 2, one with it at 63 and 130, and one
    with it at all four offsets of line 4 -- '>' too, which cannot lead line 2 but may stand inside it.  The other bases
    are cut from `genome` (random without one) with a substitution next to every placement, so that the value's neighbours
    are candidates of a correction; the other qualities are 50 .. 73, one in eight below the threshold byte 53."""
    rng = np.random.default_rng(940)
    source = np.frombuffer(genome, dtype=np.uint8) if genome else BASES[rng.integers(0, 4, 4000)]
    assert source.size >= WALKER_LEN
    out = []
    for b in range(256):
        if b in (10, 13):
            continue
        for where, in_qual in (((10, 64), False), ((63, 130), False), (WALKER_AT, True)):
            at = int(rng.integers(0, source.size - WALKER_LEN + 1))
            seq = source[at:at + WALKER_LEN].copy()
            qual = rng.integers(50, 74, WALKER_LEN).astype(np.uint8)
            for p in where:
                for near in (p - 2, p + 3):                  # a wrong base on either side, within reach of any k >= 5
                    seq[near] = BASES[(int(np.flatnonzero(BASES == (seq[near] & 0xDF))[0]) + 1 + int(rng.integers(0, 3))) % 4] | (seq[near] & 0x20)
                (qual if in_qual else seq)[p] = b
            out.append(b"@w%d %d\n" % (b, where[0]) + seq.tobytes() + b"\n+\n" + qual.tobytes() + b"\n")
    text = b"".join(out)
    assert len(text) < 1_000_000
    return text
