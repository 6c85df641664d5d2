"""Seeded test inputs shared by oracle/gen_golden.py (which ran the reference on them) and the tests.

Every golden fixture names its input by a small spec dict; `make_input(spec)` rebuilds the exact
bytes (checked against the sha256 stored in the manifest), so only expected outputs are committed.
"""
import gzip
import hashlib
import io
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def kat_fasta(k: int) -> bytes:
    """Every one of the 4^k k-mers as its own record -- the layout /root/reference/test.py:8-27 writes
    (header `>examples/example--KK-NNNNNNNNNN`, one k-mer per record, lexicographic ACGT order)."""
    out = io.BytesIO()
    for num, tup in enumerate(itertools.product("ACGT", repeat=k)):
        out.write(f">examples/example--{k:02d}-{num + 1:010d}\n{''.join(tup)}\n".encode())
    return out.getvalue()


def edge_fasta() -> bytes:
    """Hand-built FASTA exercising every parser corner SURVEY.md 8c lists (G3)."""
    state = [12345]

    def nxt():                                   # splitmix64: no dependence on numpy's generators
        state[0] = (state[0] + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = state[0]
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)

    def rand(n, alphabet="ACGT"):
        return "".join(alphabet[(nxt() >> 33) % len(alphabet)] for _ in range(n))

    def wrap(s, w=60, eol="\n"):
        return eol.join(s[i:i + w] for i in range(0, len(s), w)) + eol

    p = []
    p.append("ACGTACGTACGTACGTACGTACGT\nthis text precedes the first header and is dropped\n")
    p.append(">rec01 plain uppercase with a description  \n" + wrap(rand(3000)))
    p.append(">rec02_lowercase\n" + wrap(rand(1500, "acgt")))
    p.append(">rec03_mixed_case_and_N_runs\n" + wrap(rand(400) + "N" * 37 + rand(300, "acgt") + "n" * 5 + rand(700) + "N" + rand(90)))
    p.append(">rec04_iupac\n" + wrap(rand(200) + "RYKMSWBDHVN" + rand(200) + "ryk" + rand(100) + "U" + rand(50) + "-*." + rand(64)))
    p.append(">rec05_crlf\r\n" + wrap(rand(900), 70, "\r\n"))
    p.append(">rec06_blank_lines\n\n\n" + rand(80) + "\n\n   \n\t\n" + rand(75) + "\n\n")
    p.append(">rec07_lead_trail_ws\n   " + rand(60) + "\n" + rand(60) + "   \t\n\t " + rand(45) + " \n")
    p.append(">rec08_interior_space\n" + rand(40) + " " + rand(40) + "\n" + rand(30) + "\t\t" + rand(30) + "\n")
    p.append(">rec09_empty\n")
    p.append(">rec10_shorter_than_k\nACGTA\n")
    p.append(">rec11_exactly_7\nACGTTGC\n")
    p.append(">rec12_exactly_15\nACGTTGCAAGCTTAG\n")
    p.append(">rec13_all_N\n" + wrap("N" * 333))
    p.append(">rec14 gt mid-line\n" + rand(50) + ">" + rand(50) + "\n")
    p.append(">rec15_polyA\n" + wrap("A" * 700 + rand(20) + "T" * 400))
    p.append(">rec16_microsat\n" + wrap("AT" * 300 + rand(33) + "AAG" * 250 + rand(10) + "ACGT" * 100))
    p.append(">rec17_lone_cr\r" + rand(100) + "\r" + rand(77) + "\r")
    p.append("  \t>rec18_header_with_leading_ws\n" + wrap(rand(500)))
    p.append(">rec19_vt_ff_fs\n" + rand(50) + "\x0b\n\x0c" + rand(50) + "\x1c\n" + rand(20) + "\x0b" + rand(20) + "\n")
    p.append(">\n" + wrap(rand(120)))                       # empty name
    p.append(">rec21_kmers_only_across_lines\nACG\nTAC\nGTA\nCGT\nACG\nTTG\n")
    p.append(">rec22_saturation\n" + wrap(("ACGTTGCAAGCTTAGGCTAACGTAT" + "C") * 300))
    p.append(">rec23_no_trailing_newline\n" + rand(500))     # last line has no \n
    return "".join(p).encode("ascii")


def make_input(spec: dict) -> bytes:
    kind = spec["gen"]
    if kind == "kat":
        data = kat_fasta(spec["k"])
    elif kind == "edge":
        data = edge_fasta()
    elif kind == "edge_gz":
        data = gzip.compress(edge_fasta(), mtime=0)
    elif kind == "c1":
        data = synth.c1(**spec.get("args", {}))[0].tobytes()
    elif kind == "c2":
        data = synth.c2(**spec.get("args", {}))[0].tobytes()
    elif kind == "family":
        data = synth.family(**spec["args"])[0].tobytes()
    elif kind == "bgzf_table":                        # a count-table-like byte string: mostly zeros, small counts (seeded, numpy-free stream)
        import struct
        x, out = spec["seed"] * 0x9E3779B97F4A7C15 & 0xFFFFFFFFFFFFFFFF, bytearray()
        for _ in range(spec["n"]):
            x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
            r = x >> 40
            out.append(0 if r % 10 < 7 else 1 + (r >> 8) % 5)
        data = bytes(out)
    else:
        raise KeyError(kind)
    return data


def skewed_fasta(n_bp: int, unit_len: int, seed: int = 7, stretch: int = 2048, chunk: int = 16384, stride: int = 16,
                 width=60) -> bytes:
    """One record that defeats the bucket-size sample on purpose.  The indexer sizes its buckets from one wave's stretch
    of bases (`stretch`: 64 threads x 32 bases for 32-bit k-mers, x 16 for 64-bit ones) out of every `stride` stretches:
    stretch number q of the text's 16 KiB chunks is sampled iff q % stride == (q // stride) % stride (kmer_fuse.hip,
    locate).  Here exactly those stretches hold uniform random sequence and everything else repeats one `unit_len`-base
    unit (a period the hot-key path does not look for), so the estimate is wrong by an order of magnitude, the buckets
    overflow and the exact re-layout has to run.  `width`: bases per line (None: the whole sequence on one line)."""
    import numpy as np
    width = n_bp if width is None else width
    assert n_bp % width == 0 and chunk % stretch == 0
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    head = b">skewed_against_the_sample\n"
    i = np.arange(n_bp, dtype=np.int64)
    sampled = _sampled_bases(len(head), n_bp, width, stretch, chunk, stride)
    unit = acgt[rng.integers(0, 4, size=unit_len)]
    seq = acgt[rng.integers(0, 4, size=n_bp)]
    rep = ~sampled
    seq[rep] = unit[i[rep] % unit_len]
    return head + _lines(seq, width)


def _base_offsets(head_len: int, n_bp: int, width: int):
    import numpy as np
    i = np.arange(n_bp, dtype=np.int64)
    return i, head_len + i + i // width                         # byte offset of base i: `width` bases and a newline per line


def _sampled_bases(head_len: int, n_bp: int, width: int, stretch: int = 2048, chunk: int = 16384, stride: int = 16):
    """Which bases of a one-record text (a `head_len`-byte header, then lines of `width` bases) the bucket-size sample sees."""
    import numpy as np
    i, off = _base_offsets(head_len, n_bp, width)
    slot = off // chunk
    first = np.searchsorted(slot, np.arange(slot[-1] + 1))     # index of the first base of every chunk
    q = slot * (chunk // stretch) + (i - first[slot]) // stretch
    return q % stride == (q // stride) % stride


def _lines(seq, width: int) -> bytes:
    import numpy as np
    lines = np.empty((seq.size // width, width + 1), dtype=np.uint8)
    lines[:, :width] = seq.reshape(-1, width)
    lines[:, width] = 10
    return lines.tobytes()


def headers_on_lines(text: bytes, head_len: int, width: int, line_idx, tag: bytes = b"r") -> bytes:
    """`text` (a `head_len`-byte header, then lines of `width` bases) with the given sequence lines replaced by header lines
    of the same length: every byte offset stays where it was, every replaced line opens a record."""
    import numpy as np
    body = np.frombuffer(text, dtype=np.uint8, offset=head_len).reshape(-1, width + 1).copy()
    line_idx = np.asarray(line_idx, dtype=np.int64)
    heads = b"".join((b">%s%d_" % (tag, n)).ljust(width, b"x") for n in range(line_idx.size))
    body[line_idx, :width] = np.frombuffer(heads, dtype=np.uint8).reshape(-1, width)
    return text[:head_len] + body.tobytes()


def record_dense_fasta(n_bytes: int, every: int, seed: int = 5, head_len: int = 27, width: int = 60) -> bytes:
    """Random sequence of exactly `n_bytes` bytes laid out like skewed_fasta (a `head_len`-byte header line, then lines of
    `width` bases), every `every`-th line a header of the same length: many short records of ordinary sequence."""
    import numpy as np
    n_lines = (n_bytes - head_len) // (width + 1)
    assert head_len + n_lines * (width + 1) == n_bytes
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n_lines * width)]
    head = b">dense".ljust(head_len - 1, b"_") + b"\n"
    text = head + _lines(seq, width)
    return headers_on_lines(text, head_len, width, np.arange(every - 1, n_lines, every), tag=b"d")


def skewed_fasta_with_records(n_bp: int, unit_len: int, n_records: int, seed: int = 7, stretch: int = 2048,
                              chunk: int = 16384, stride: int = 16) -> bytes:
    """skewed_fasta(n_bp, unit_len, ...) with `n_records` of its lines turned into header lines of the same length, all of
    them behind the last sampled base of their 16 KiB chunk: what the sample sees -- every sampled base at the same
    place in its chunk's squeezed bases -- stays as it was, so the text still defeats the sample, and it also brings
    `n_records` + 1 records."""
    import numpy as np
    text = skewed_fasta(n_bp, unit_len, seed=seed, stretch=stretch, chunk=chunk, stride=stride)
    head_len = len(b">skewed_against_the_sample\n")
    sampled = _sampled_bases(head_len, n_bp, 60, stretch, chunk, stride)
    i, off = _base_offsets(head_len, n_bp, 60)
    n_chunks = int(off[-1] // chunk) + 1
    last = np.full(n_chunks, -1, dtype=np.int64)                # offset of the last sampled base of every chunk
    np.maximum.at(last, off[sampled] // chunk, off[sampled])
    line_start = head_len + np.arange(n_bp // 60, dtype=np.int64) * 61
    c0, c1 = line_start // chunk, (line_start + 60) // chunk     # chunks of the line's first byte and of its newline
    ok = np.flatnonzero((c0 == c1) & (line_start > last[c0]))
    assert ok.size >= n_records, (ok.size, n_records)
    pick = ok[np.linspace(0, ok.size - 1, n_records).astype(np.int64)]
    return headers_on_lines(text, head_len, 60, np.unique(pick), tag=b"s")


def interspersed_repeat(n_copies, unit_len, spacer, seed):
    """`n_copies` of one unit, each followed by `spacer` random bases: every k-mer of the unit occurs n_copies times, but
    never with a period of 1-3 bases (the hot-key path does not see it) and never as a long run of records in one bucket."""
    import numpy as np
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    unit = acgt[rng.integers(0, 4, size=unit_len)]
    parts = []
    for _ in range(n_copies):
        parts.append(unit)
        parts.append(acgt[rng.integers(0, 4, size=spacer)])
    seq = np.concatenate(parts)
    seq = seq[: seq.size // 60 * 60]
    return b">interspersed\n" + _lines(seq, 60)


SOUP_ALPHABET = b"ACGTacgtNn>> \t\r\n\n\n\x0b\x0cXR"


def byte_soup(n: int, seed: int) -> bytes:
    """Random bytes over the FASTA-relevant alphabet (the soup of test_random_structure_fuzz), behind one header so that
    none of it is text in front of the first record."""
    import numpy as np
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(SOUP_ALPHABET, dtype=np.uint8)
    w = rng.random(alphabet.size) ** 3
    return b">soup\n" + alphabet[rng.choice(alphabet.size, size=n, p=w / w.sum())].tobytes()


# ------------------------------------------------------------------ deep windows (k = 19, 21) ------------------------
# The window that reaches furthest back across a seam (a 16 KiB slot boundary, or the end of a feed) is the one that
# needs the most history.  The builders below write SEAM_MOTIF where that window begins, so that its canonical k-mer --
# the forward one unless the window happens to end in the motif's reverse complement -- has the same leading bases at
# every seam and the seams of a text share one address slice (the tests assert it from the oracle).
SEAM_MOTIF = b"ACGA"


def _rand_bases(rng, n: int) -> bytes:
    import numpy as np
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def deep_seam_fasta(k: int, seed: int = 19, pad_to_chunks: int = 0, chunk: int = 16384):
    """(text, sites): one record whose 16 KiB chunk boundaries meet every carried run the deep-window kernel tells apart.
    `sites` lists (kind, d, offset): at byte `offset` (a multiple of `chunk`) a base follows that has exactly `d` valid
    bases behind it since the last restart -- or, for the shapes, a long run whose newest bases lie some slots back:

      "line", d = 0 .. k + 3           (not a boundary) d bases behind a line start inside a long run: a place to cut a feed;
      "N" / "header", d = 0 .. k + 3   the restart is an N / a header line, d bases before the boundary;
      "newlines" / "blanks"            a whole chunk of line terminators / of trailing blanks in front (no base in it);
      "thin", d = j                    two empty chunks, a chunk with j bases, an empty chunk: history from >= 3 slots;
      "long_header"                    a 40 000-byte header line in front: three chunks without a base and a restart;
      "one_base_lines", "crlf"         lines of one base (8192 bases per slot) / CR LF lines across three boundaries.

    Where the oldest window that crosses the boundary begins, the text holds SEAM_MOTIF.  `pad_to_chunks`: plain sequence
    lines are appended until the text has that many chunks."""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = bytearray(b">deep_seams\n")
    sites = []

    def fill_to(target):                                    # sequence lines of <= 60 bases up to exactly `target`, ending in a newline
        n = target - len(out)
        assert n >= 1, (target, len(out))
        while n > 0:
            m = min(61, n)
            out.extend(_rand_bases(rng, m - 1) + b"\n")
            n -= m

    def boundary(margin=400):
        return (len(out) + margin + chunk - 1) // chunk * chunk

    def run_up_to(B, back=k - 1, n=30):                      # n bases on one line that end right at B, the motif `back` bases before B
        fill_to(B - n)
        tail = bytearray(_rand_bases(rng, n))
        if back >= len(SEAM_MOTIF):
            tail[n - back: n - back + len(SEAM_MOTIF)] = SEAM_MOTIF
        out.extend(tail)
        assert len(out) == B

    fill_to(12 + 61 * 120)                                   # plain lines of 60 bases: line i begins at 12 + 61 i
    for d in range(0, k + 4):                                # "line": d bases behind a line start inside a long run
        cut = 12 + 61 * (5 + 4 * d) + d
        at, left = cut, k - 1
        while left:                                          # k - 1 bases back, over the newline
            at -= 1
            left -= out[at] != 10
        for ch in SEAM_MOTIF:
            at += out[at] == 10
            out[at] = ch
            at += 1
        sites.append(("line", d, cut))
    for kind in ("N", "header"):
        for d in range(0, k + 4):
            B = boundary()
            marker = b"N" if kind == "N" else b">h%d\n" % d
            if kind == "N":
                fill_to(B - d - 1 - 30)
                out.extend(_rand_bases(rng, 30))
            else:
                fill_to(B - d - len(marker))
            run = bytearray(_rand_bases(rng, d + 40))        # d bases, the boundary, 40 more on the same line
            at = max(0, d - (k - 1))                         # where the oldest window across the boundary begins
            run[at: at + len(SEAM_MOTIF)] = SEAM_MOTIF
            out.extend(marker + bytes(run) + b"\n")
            assert len(out) == B + 41
            sites.append((kind, d, B))
    for kind, gap in (("newlines", b"\n" * chunk), ("blanks", b" " * (chunk - 1) + b"\n")):
        B = boundary()
        run_up_to(B)
        out.extend(gap + _rand_bases(rng, 40) + b"\n")
        sites.append((kind, k - 1, B + chunk))
    for j in (1, 2, 7, 15, 16, 17, 20, 31):
        B = boundary()
        run_up_to(B, k - 1 - j)                              # the oldest window across the last boundary: j bases of the thin chunk + k-1-j from here
        thin = bytearray(_rand_bases(rng, j))
        if 0 <= j - (k - 1) <= j - len(SEAM_MOTIF):
            thin[j - (k - 1): j - (k - 1) + len(SEAM_MOTIF)] = SEAM_MOTIF
        out.extend(b"\n" * (2 * chunk) + bytes(thin) + b"\n" * (chunk - j) + b"\n" * chunk + _rand_bases(rng, 40) + b"\n")
        sites.append(("thin", j, B + 4 * chunk))
    B = boundary()
    run_up_to(B - 1)
    out.extend(b"\n>" + b"H" * 40000 + b"\n")
    at = len(out)
    out.extend(SEAM_MOTIF + _rand_bases(rng, 3 * chunk - 40002 - 1 - len(SEAM_MOTIF)) + b"\n")   # the record's first bases, on one line up to a boundary
    sites.append(("long_header", 0, at))
    B = boundary()
    fill_to(B)
    one = np.empty((3 * chunk // 2, 2), dtype=np.uint8)
    one[:, 0] = np.frombuffer(_rand_bases(rng, one.shape[0]), dtype=np.uint8)
    one[:, 1] = 10
    out.extend(one.tobytes())
    sites.append(("one_base_lines", k - 1, B + chunk))
    B = boundary()
    fill_to(B)
    while len(out) < B + 3 * chunk:
        out.extend(_rand_bases(rng, 70) + b"\r\n")
    sites.append(("crlf", k - 1, B + chunk))
    fill_to(max(boundary(), pad_to_chunks * chunk - 100))
    out.extend(_rand_bases(rng, 57))                         # no newline at the end
    return bytes(out), sites


# ------------------------------------------------------------------ scan-tile seams (1024 chunks) -------------------
# Per-chunk summaries are combined across a feed in tiles of 1024 chunks (SCAN_T, kmer_count.hip; k_query_scan and
# k_fq_scan walk 1024 at a time too): byte TILE * t of a feed is where a tile seed, not a neighbouring thread, hands the
# parser state on.
TILE = 1024 * 16384
TILE_HEADER = b">tile_seams\n"
TINY_RECORDS = 400
TINY_BASES = b"ACGTTGCAAGCTTAGGCTAACGTAT"


def tile_site_kinds(k: int) -> list:
    """Every (kind, d) that tile_seam_fasta writes."""
    return ([("header_across", d) for d in (1, 2, 63, 64, 65, 20000)] + [("header_at", 0), ("header_ends", 0), ("crlf_split", 0), ("blank_gt", 0)]
            + [("pending_blanks_base", d) for d in (1, 40)] + [("pending_blanks_eol", d) for d in (1, 40)]
            + [("N", d) for d in (0, 1, k - 2, k - 1, k, k + 3)] + [("empty_chunks", 0), ("tiny_records", 0)])


def _fill_lines(rng, n: int) -> bytes:
    """Exactly n bytes (n >= 2) of random sequence lines of at most 60 bases, each with its newline."""
    import numpy as np
    assert n >= 2, n
    full, rest = divmod(n, 61)
    if rest == 1:                                            # no line of a newline alone: 61 + 1 = 31 + 31
        full, rest = full - 1, 62
        assert full >= 0
    short = b""
    if rest == 62:
        short = _rand_bases(rng, 30) + b"\n" + _rand_bases(rng, 30) + b"\n"
    elif rest:
        short = _rand_bases(rng, rest - 1) + b"\n"
    seq = np.frombuffer(_rand_bases(rng, full * 60), dtype=np.uint8)
    return short + _lines(seq, 60)


def _with_motif(bases: bytes, at: int) -> bytes:
    out = bytearray(bases)
    out[at: at + len(SEAM_MOTIF)] = SEAM_MOTIF
    assert len(out) == len(bases)
    return bytes(out)


def _tile_site(rng, k: int, kind: str, d: int, B: int):
    """(pre, post, plan): the bytes that end at B, the bytes that begin there (they end with a newline), and what the site
    is meant to be: `crossing` valid windows begin in front of B and end at or behind it, the oldest `reach` bases in front;
    `span`: the bytes the site wrote; `records`: (name_off, name,
    seq_len or None) of the records the site opens (seq_len where the record also ends inside the site)."""
    def run_line(n):                                         # n bases and a newline, SEAM_MOTIF first
        return _with_motif(_rand_bases(rng, n), 0) + b"\n"

    recs, crossing = [], 0
    if kind == "header_across":                              # '>' d bytes before B, the line ends behind B
        name = (b"across_d%d_" % d).ljust(d + 11, b"h")
        pre, post = (b">" + name)[:d], (b">" + name)[d:] + b"\n" + run_line(60)
        recs.append((B - d + 1, name, None))
    elif kind == "header_at":                                # a sequence line ends with the tile, '>' opens the next one
        pre, post = b"", b">at_the_seam\n" + run_line(60)
        recs.append((B + 1, b"at_the_seam", None))
    elif kind == "header_ends":                              # the header's newline is the tile's last byte
        pre, post = b">ends_with_the_tile\n", run_line(60)
        recs.append((B - len(pre) + 1, b"ends_with_the_tile", None))
    elif kind == "crlf_split":                               # CR at B - 1, LF at B
        lines = [_rand_bases(rng, 60) for _ in range(10)]
        lines[4] = _with_motif(lines[4], 60 - (k - 1))
        pre = b">crlf_lines\r\n" + b"\r\n".join(lines[:5]) + b"\r"
        post = b"\n" + b"\r\n".join(lines[5:]) + b"\r\n"
        recs.append((B - len(pre) + 1, b"crlf_lines", None))
        crossing = k - 1
    elif kind == "blank_gt":                                 # the line is still at its start when the seam comes
        pre, post = b"  \t", b">blank_gt name\n" + run_line(60)
        recs.append((B + 1, b"blank_gt name", None))
    elif kind == "pending_blanks_base":                      # interior blanks: they count as sequence and break the run
        pre, post = _rand_bases(rng, 30) + b" " * d, run_line(40)
    elif kind == "pending_blanks_eol":                       # trailing blanks: stripped, the run goes on in the next line
        pre, post = _with_motif(_rand_bases(rng, 30), 30 - (k - 1)) + b" " * d, b"\n" + _rand_bases(rng, 60) + b"\n"
        crossing = k - 1
    elif kind == "N":                                        # d valid bases between an N and B, the line goes on
        run = _with_motif(_rand_bases(rng, d + 40), max(0, d - (k - 1)))
        pre, post = _rand_bases(rng, 30) + b"N" + run[:d], run[d:] + b"\n"
        crossing = min(d, k - 1)
    elif kind == "empty_chunks":                             # the newest bases lie three chunks back
        pre, post = _with_motif(_rand_bases(rng, 30), 30 - (k - 1)) + b"\n" * (2 * 16384), _rand_bases(rng, 40) + b"\n"
        crossing = k - 1
    elif kind == "tiny_records":                             # record number TINY_RECORDS / 2 - 1 lies across B
        half = TINY_RECORDS // 2
        texts = []
        for i in range(TINY_RECORDS):
            n = k + 1 if i == half - 1 else i % (k + 2)
            seq = _with_motif(_rand_bases(rng, n), 0) if i == half - 1 else (TINY_BASES * 2)[:n]
            texts.append((b">t%d\n" % i, seq))
        pre = b"".join(h + s + b"\n" for h, s in texts[:half - 1]) + texts[half - 1][0] + texts[half - 1][1][:k - 1]
        post = texts[half - 1][1][k - 1:] + b"\n" + b"".join(h + s + b"\n" for h, s in texts[half:]) + b">behind_the_tiny_records\n"
        at = B - len(pre)
        for h, s in texts:
            recs.append((at + 1, h[1:-1], len(s)))
            at += len(h) + len(s) + 1
        recs.append((at + 1, b"behind_the_tiny_records", None))
        crossing = 2                                         # k + 1 bases, k - 1 of them in front of B: both windows cross
        assert len(pre) <= 4000 and len(post) <= 4000
    else:
        raise KeyError(kind)
    reach = k - 1 if kind == "tiny_records" else crossing    # bases in front of B of the oldest window across it
    return pre, post, {"crossing": crossing, "reach": reach, "records": recs, "span": (B - len(pre), B + len(post))}


def tile_seam_fasta(k: int, sites_at, seed: int, plan: dict = None, n_bytes: int = None, gap_chunks: int = 16):
    """(text, sites): ordinary 60-column sequence lines with one site per entry (kind, d, offset) of `sites_at`; `offset`
    is a byte offset of the text -- the caller puts it on a multiple of TILE of the feed it will lie in.  What the text
    holds at B = offset (tile_site_kinds lists the kinds):

      "header_across", d     '>' d bytes before B, the header line ends behind B (d = 20000: it fills the tile's last chunk);
      "header_at"            a line terminator is the last byte before B, '>' the byte at B;
      "header_ends"          a header's terminator is the last byte before B, bases begin at B;
      "crlf_split"           CR at B - 1, LF at B, inside a record of CR LF lines;
      "blank_gt"             a line "  \t>name", its blanks in front of B and '>' at B;
      "pending_blanks_base", d   d blanks in front of B inside a sequence line, a base at B: the run breaks;
      "pending_blanks_eol", d    d blanks in front of B, the terminator at B: trailing blanks, the run goes on;
      "N", d                 exactly d valid bases between an N and B, the run goes on behind B on the same line;
      "empty_chunks"         the two chunks in front of B are all newlines, the bases behind B continue the run from before;
      "tiny_records"         TINY_RECORDS records `>tN` of 0 .. k + 1 bases around B, one of them across it, and a header
                             behind them.

    Where the oldest window that crosses B begins -- or, where none does, the first one behind B -- the text holds
    SEAM_MOTIF.  The text ends without a newline, 16 chunks behind the last site or, if given, after `n_bytes` bytes.
    `plan`, if given, receives per site what _tile_site planned; `gap_chunks`: the least run of plain sequence lines between
    two sites (a text of a prescribed size may not have room for 16 chunks)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    parts, pos, sites = [TILE_HEADER], len(TILE_HEADER), []
    for kind, d, B in sorted(sites_at, key=lambda s: s[2]):
        pre, post, p = _tile_site(rng, k, kind, d, B)
        assert B - len(pre) - pos >= gap_chunks * 16384, "chunks of plain sequence in front of every site"
        parts.append(_fill_lines(rng, B - len(pre) - pos))
        parts += [pre, post]
        pos = B + len(post)
        sites.append((kind, d, B))
        if plan is not None:
            plan[(kind, d, B)] = p
    end = n_bytes if n_bytes is not None else pos + 16 * 16384 + 57
    assert end - 57 - pos >= 2 * 16384, "plain sequence behind the last site"
    parts.append(_fill_lines(rng, end - 57 - pos))
    parts.append(_rand_bases(rng, 57))                       # no newline at the end
    return b"".join(parts), sites


def tile_cases(k: int) -> list:
    """tile_site_kinds(k) in cases of at most four sites: case i puts its sites on bytes TILE, 2 TILE, ... of one feed."""
    kinds = tile_site_kinds(k)
    return [[(kind, d, TILE * (j + 1)) for j, (kind, d) in enumerate(kinds[i:i + 4])] for i in range(0, len(kinds), 4)]


TILE_FEEDS = (TILE + 3 * 16384 + 7, TILE + 5 * 16384)       # two feeds of more than 1024 chunks each


def tile_second_feed_cases(k: int) -> list:
    """Two-site cases for a text fed as TILE_FEEDS: one site of every kind on the second feed's own tile seam (byte
    TILE_FEEDS[0] + TILE of the text), and one of the remaining (kind, d) on the first feed's."""
    second = [("header_across", 1), ("header_across", 20000), ("header_at", 0), ("header_ends", 0), ("crlf_split", 0), ("blank_gt", 0),
              ("pending_blanks_base", 40), ("pending_blanks_eol", 40), ("N", k - 1), ("empty_chunks", 0), ("tiny_records", 0)]
    first = [s for s in tile_site_kinds(k) if s not in second]
    assert len(first) == len(second)
    return [[(*a, TILE), (*b, TILE_FEEDS[0] + TILE)] for a, b in zip(first, second)]


def tile_deep_sites(k: int) -> list:
    """The sites of the deep-window cases (k = 19, 21), each on byte TILE of a text of its own."""
    return [("N", k - 1, TILE), ("N", k + 3, TILE), ("empty_chunks", 0, TILE)]


QUERY_TILE_BYTES = 2 * TILE + 5 * 16384
QUERY_TILE_CUT = TILE + 2 * 16384 + 7                       # two feeds of more than 1024 chunks each


def tile_query_sites(k: int) -> list:
    """Sites of the query text: chunks 1024 and 2048 of the text, and chunk 1024 of its second feed when it is cut at
    QUERY_TILE_CUT.  The record that opens the text runs on across chunk 1024 (the N site lies inside it)."""
    return [("N", k - 1, TILE), ("tiny_records", 0, QUERY_TILE_CUT + TILE), ("header_across", 65, 2 * TILE)]


def plain_sequence_fasta(n_bp: int, seed: int = 3, n_at=(), motif_at=()):
    """One record, its `n_bp` bases on ONE line.  `n_at`: byte offsets that hold an N instead; `motif_at`: byte offsets where
    SEAM_MOTIF is written.  Bytes: a 7-byte header line, base i at offset 7 + i."""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = bytearray(b">plain\n" + _rand_bases(rng, n_bp) + b"\n")
    for at in motif_at:
        assert at >= 7
        out[at: at + len(SEAM_MOTIF)] = SEAM_MOTIF
    for x in n_at:
        out[x] = ord("N")
    return bytes(out)


def deep_tandem_fasta(k: int, seed: int, n_runs: int = 12000) -> bytes:
    """Thousands of tandem runs of period 1, 2 and 3 and of k - 2 .. k + 40 bases, between spacers of 0 .. 5 bases (so they
    start at every offset of a code word and cross slot boundaries), an N inside some of them; then runs of A, AT, AAG
    and ACGT long enough to saturate their addresses."""
    import numpy as np
    rng = np.random.default_rng(seed)
    parts, line = [b">deep_tandems\n"], []
    for i in range(n_runs):
        period = 1 + i % 3
        motif = _rand_bases(rng, period)
        n = int(rng.integers(k - 2, k + 41))
        run = bytearray((motif * (n // period + 1))[:n])
        if i % 7 == 0:
            run[int(rng.integers(n))] = ord("N")
        line.append(bytes(run) + _rand_bases(rng, int(rng.integers(0, 6))))
        if len(line) == 3:
            parts.append(b"".join(line) + b"\n")
            line = []
    parts.append(b"".join(line) + b"\n")
    parts.append(b">long_runs\n" + b"A" * 40000 + b"\n" + b"AT" * 12000 + b"\n" + b"AAG" * 9000 + b"\n" + b"ACGT" * 7000 + b"\n")
    return b"".join(parts)


def deep_k21_fasta(seed: int = 2121, body_bp: int = 300_000):
    """The k = 21 slice text: the parser corners of edge_fasta, a synthetic body with tandem repeats, duplications, N gaps
    and lower case, poly-A (address 0 saturates) and windows whose k-mer AND reverse complement begin with TTTT (the last
    of 256 slices).  `body_bp`: size of the synthetic body (0: none; even 30 kbp of text leave hardly any of the 256 slices empty)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    body = synth.generate(94, body_bp, 3, pm_tandem=100, pm_dup=100, pm_ngap=30, pm_lower=50)[0] if body_bp else np.zeros(0, dtype=np.uint8)
    top = b"N".join(b"TTTT" + _rand_bases(rng, 13) + b"AAAA" for _ in range(40))
    tail = b">polyA\n" + b"A" * 800 + b"\n" + b"ACGT" * 200 + b"\n>top_slice\n" + top + b"\n" + (b"TTTTGCATGCATGCATGAAAA" + b"N") * 300 + b"\n"
    return edge_fasta() + body.tobytes() + tail


def sha256(data) -> str:
    return hashlib.sha256(data).hexdigest()


# ------------------------------------------------------------------ feeds that overflow the record array
RECS_INITIAL = 4096                                          # pk_indexer_create_slice: record slots of a fresh indexer


def record_overflows(lengths, record_starts):
    """Which of the feeds (byte lengths, in order; 0 = an empty feed, which never reaches the pipeline) bring more records
    than the record array holds when they arrive -- the capacity rule of pk_indexer.hip (ensure_recs, run_feed: after every
    feed room for as many records again as it brought, times two, + 1024).  `record_starts`: offset of every record's '>'."""
    import numpy as np
    starts = np.sort(np.asarray(record_starts, dtype=np.int64))
    cap, n, end, out = RECS_INITIAL, 0, 0, []

    def grown(cap, need):
        return cap if need <= cap else max(need, max(1024, 2 * cap))

    for length in lengths:
        if length == 0:
            out.append(False)
            continue
        end += length
        n_after = int(np.searchsorted(starts, end))
        out.append(n_after > cap)
        cap = grown(cap, n_after)
        cap = grown(cap, n_after + 2 * (n_after - n) + 1024)
        n = n_after
    return out


def record_starts(records):
    """The offset of every record's '>' from the records of a count."""
    import numpy as np
    return records["name_off"].astype(np.int64) - 1
