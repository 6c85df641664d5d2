"""CPU: the conditions that the streams of record_feed_inputs must meet for test_gpu_record_feeds.py to reach what it is
there for, asserted from the references alone -- the constants of the kernels the streams are built around (4096 =
TRIM_SCAN_T * TRIM_SCAN_PER, 32 768 = TRIM_MAX_WGS * TRIM_WAVES, TRIM_ROUND = 256), read out of kmer_trim.h and kmer_trim.hip;
mixed cover bits around every scan round's first record; every outcome class in the grid's second and third pass; long
reads in front of corrected ones in the same wave; a lost scan carry changes `covered`; the long lines, blank runs and read
lengths of the long-line stream and corrected candidates far into its reads -- and trim.RecordFeeds on records of up to and
beyond two blocks."""
import os
import re

import numpy as np
import pytest

import record_feed_inputs as rfi
import trim_ref
from correct_inputs import BLANKS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("untried", "corrected", "ambiguous", "unfixable")


def _constant(text: str, name: str) -> str:
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text)
    assert m, name
    return m.group(1).strip()


def test_the_streams_are_built_around_the_kernels_constants():
    h = open(os.path.join(ROOT, "pykmer_amd", "csrc", "kmer_trim.h")).read()
    hip = open(os.path.join(ROOT, "pykmer_amd", "csrc", "kmer_trim.hip")).read()
    wg = int(_constant(open(os.path.join(ROOT, "pykmer_amd", "csrc", "fasta_fsm.h")).read(), "WG"))    # TRIM_WAVES = WG / 64
    assert _constant(h, "TRIM_WAVES") == "WG / 64" and _constant(h, "TRIM_ROUND") == "64u * TRIM_STEPS"
    waves, steps, max_wgs = wg // 64, int(_constant(h, "TRIM_STEPS")), int(_constant(h, "TRIM_MAX_WGS"))
    assert int(_constant(hip, "TRIM_SCAN_T")) * int(_constant(hip, "TRIM_SCAN_PER")) == rfi.SCAN_ROUND == 4096
    assert max_wgs * waves == rfi.STRIDE == 32768
    assert 64 * steps == rfi.ROUND == 256
    assert rfi.R_MANY > 2 * rfi.STRIDE + 1000 and len(rfi.seams()) + 1 == 18 and {rfi.STRIDE, 2 * rfi.STRIDE} <= set(rfi.seams())


# ------------------------------------------------------------------ the many-record stream
def _firsts(n_valid):
    return np.concatenate([[0], np.cumsum(n_valid.astype(np.int64))])


@pytest.mark.parametrize("which", ["trim", "correct"])
def test_many_records_mixed_bits_around_every_scan_round(which):
    want = rfi.many_trim() if which == "trim" else rfi.many_correct()
    assert want["seq_len"].size == rfi.R_MANY == len(rfi.many_starts()) - 1
    first = _firsts(want["n_valid_bases"])
    assert int(first[-1]) == want["n_bases"] == want["cover"].size
    for b in rfi.seams():
        for r in (b - 1, b, b + 1):
            bits = want["cover"][first[r]:first[r + 1]]
            assert bits.size >= 8 and 0 < int(bits.sum()) < bits.size, (which, b, r, bits)


def test_many_records_every_class_in_every_pass_of_the_grid():
    want = rfi.many_correct()
    counts = {name: int(want[name].sum()) for name in CLASSES + ("candidates",)}
    assert min(counts.values()) >= 1000, counts
    for lo in (rfi.STRIDE, 2 * rfi.STRIDE):
        late = {name: int(want[name][lo:].sum()) for name in CLASSES}
        assert min(late.values()) >= 100, (lo, late)
    r = np.arange(rfi.R_MANY - rfi.STRIDE)
    pairs = (want["n_valid_bases"][r] >= 129) & (want["corrected"][r + rfi.STRIDE] > 0)      # a full ring, then a corrected base
    assert int(pairs.sum()) >= 20, int(pairs.sum())
    lengths = set(want["seq_len"].tolist())
    assert set(range(0, 2 * rfi.K_MANY + 3)) | set(rfi.LONG) <= lengths
    assert int((want["seq_len"] != want["n_valid_bases"]).sum()) >= 500                      # Ns
    assert want["patched"] != rfi.many_stream() and len(want["patched"]) == len(rfi.many_stream())


def test_many_records_threshold_takes_bases_away():
    plain, low = rfi.many_trim(), rfi.many_trim(rfi.T)
    assert 0 < low["n_bases"] < plain["n_bases"] and low["seq_len"].size == rfi.R_MANY
    assert int((low["n_valid_bases"][rfi.STRIDE:] < plain["n_valid_bases"][rfi.STRIDE:]).sum()) >= 1000


@pytest.mark.parametrize("restart", [rfi.SCAN_ROUND, rfi.STRIDE])
def test_a_lost_scan_carry_would_show(restart):
    """`covered` recomputed with the ordinal of the first cover bit restarted at record `restart`, as a scan that lost its
    carry there would leave it: it must differ from the truth in many records, or the GPU test could not see such a bug."""
    want = rfi.many_trim()
    n = want["n_valid_bases"].astype(np.int64)
    first = _firsts(n)[:-1]
    ones = np.concatenate([[0], np.cumsum(want["cover"].astype(np.int64))])
    assert np.array_equal(ones[first + n] - ones[first], want["covered"].astype(np.int64))    # the formula gives the truth
    lost = first.copy()
    lost[restart:] -= first[restart]
    wrong = ones[lost + n] - ones[lost]
    assert int((wrong != want["covered"].astype(np.int64)).sum()) >= 100
    assert np.array_equal(wrong[:restart], want["covered"][:restart].astype(np.int64))


# ------------------------------------------------------------------ the long-line stream
def test_long_lines_geometry():
    k = 5
    fq, want = rfi.long_stream(k), rfi.long_trim(k)
    recs = trim_ref.record_lines(fq)
    assert len(recs) == rfi.N_LONG + 1 and not fq.endswith((b"\n", b"\r"))
    line1 = [(l1[1] - l1[0], fq[l1[1]:l1[2]]) for l1, *_ in recs]
    assert set(rfi.LINE1) <= {n for n, _ in line1}
    assert {(n, eol) for n, eol in line1 if n in rfi.LINE1} == {(n, eol) for n in rfi.LINE1 for eol in (b"\n", b"\r\n", b"\r")}
    s, e, _ = recs[next(i for i, (n, eol) in enumerate(line1) if n == 255 and eol == b"\r\n")][0]
    assert e - s == rfi.ROUND - 1 and fq[s + 255] == 13 and fq[s + 256] == 10                # \r ends a round, \n begins the next
    names = b"".join(fq[l1[0] + 1:l1[1]] for l1, *_ in recs)
    assert all(bytes([c]) in names for c in b"@+ \t\x1c\x80\xff")
    line3 = {l3[1] - l3[0] == 1 for _, _, l3, _, _ in recs}
    assert line3 == {True, False} and any(l3[1] - l3[0] == 1000 for _, _, l3, _, _ in recs)
    trail = want["end2"].astype(np.int64) - want["pos2"].astype(np.int64) - want["seq_len"].astype(np.int64)
    assert set(rfi.BLANK_RUNS) <= set(want["lead"].tolist()) and set(rfi.BLANK_RUNS) <= set(trail.tolist())
    assert set(rfi.SEQ(k)) | {rfi.GIANT} == set(want["seq_len"].tolist())
    both = set(zip(want["lead"].tolist(), trail.tolist()))
    assert len(both) >= 20 and any(a >= 255 and b >= 255 for a, b in both) and any(a == 0 and b >= 255 for a, b in both)
    # two records with 256 and 257 leading blanks by hand: record 10 has a line 1 of 511 bytes ended by \r, record 12 one of
    # 513 bytes ended by \r\n; position 0 lies behind line 1, its terminator and the blanks
    starts = rfi.long_starts(k)
    for i, l1, eol, lead in ((10, 511, b"\r", 256), (12, 513, b"\r\n", 257)):
        at = int(starts[i]) + l1 + len(eol) + lead
        assert fq[int(starts[i]) + l1:int(starts[i]) + l1 + len(eol)] == eol and fq[at - 1] in BLANKS and fq[at] in b"ACGTacgtN"
        assert (int(want["lead"][i]), int(want["pos2"][i])) == (lead, at)
        assert int(want["pos4"][i]) - int(want["end2"][i]) == len(eol) + 1 + (l1 - 1 if i % 2 else 0) + len(eol) + lead
    length = (want["trim_end"] - want["trim_start"]).astype(np.int64)
    assert int((want["trim_start"] >= 1024).sum()) >= 3 and int(((want["covered"].astype(np.int64) > length) & (length > 0)).sum()) >= 100


@pytest.mark.parametrize("k", [5, 9, 13])
def test_long_lines_hold_corrections_far_into_the_reads(k):
    want = rfi.long_correct(k)
    assert set(rfi.SEQ(k)) | {rfi.GIANT} == set(want["seq_len"].tolist())
    pos, rec = want["fix_pos"], want["fix_record"]
    for lo in (256, 512, 1024, 4096):
        assert int((pos >= lo).sum()) >= 10, (lo, int((pos >= lo).sum()))
    giant = int(np.flatnonzero(want["seq_len"] == rfi.GIANT)[0])
    assert giant == rfi.GIANT_AFTER + 1 and int(((rec == giant) & (pos > 20_000)).sum()) >= 50
    assert int(((rec != giant) & (pos >= 1024)).sum()) >= 3
    assert min(int(want[name].sum()) for name in ("untried", "corrected", "unfixable")) >= 50
    if k == 5:
        for M in (1, 2):
            other = rfi.long_correct(k, M)
            assert int(other["corrected"].sum()) > 0 and int(other["untried"].sum()) < int(want["untried"].sum())
        assert int(rfi.long_correct(k, 1)["untried"].sum()) == 0


# ------------------------------------------------------------------ trim.RecordFeeds on long records
BLOCK = 1 << 16


def _record(i: int, n_bytes: int) -> bytes:
    """A record of exactly n_bytes bytes whose bytes differ along its length."""
    head = b"@big%d\n" % i
    n = (n_bytes - len(head) - 4) // 2
    assert len(head) + 2 * n + 4 == n_bytes, "an even rest"
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(i).integers(0, 4, n)].tobytes()
    qual = (33 + np.arange(n) % 90).astype(np.uint8).tobytes()
    return head + seq + b"\n+\n" + qual + b"\n"


def _small(n_bytes: int) -> bytes:
    """Records of 100 bytes each, and a last one that fills up to n_bytes."""
    out, i = [], 0
    while n_bytes:
        size = 100 if n_bytes >= 220 else n_bytes
        name = b"@s%d" % i
        half = (size - len(name) - 5) // 2
        name += b"x" * (size - len(name) - 5 - 2 * half)
        out.append(name + b"\n" + b"A" * half + b"\n+\n" + b"I" * half + b"\n")
        assert len(out[-1]) == size
        n_bytes -= size
        i += 1
    return b"".join(out)


def _pieces(tmp_path, monkeypatch, text):
    from pykmer_amd import trim
    monkeypatch.setattr(trim, "TRIM_FEED", BLOCK)
    path = tmp_path / "long.fq"
    path.write_bytes(text)
    starts = trim_ref.starts(text)
    feeds = trim.RecordFeeds(str(path), starts)
    assert feeds.block == BLOCK
    return feeds, starts


WHOLE = [(0, 84_008), (0, 125_000), (0, 2 * BLOCK), (30_000, 84_008), (65_000, 60_000), (2 * BLOCK - 100_000, 100_000), (BLOCK - 2, BLOCK + 2),
         (BLOCK, 2 * BLOCK), (3 * BLOCK - 124_000, 124_000)]               # (the bytes in front of the record, its own)
REFUSED = [(0, 200_000), (0, 2 * BLOCK + 2), (30_000, 200_000), (30_000, 2 * BLOCK - 30_000 + 2), (BLOCK, 2 * BLOCK + 2)]


@pytest.mark.parametrize("before, size", WHOLE)
def test_record_feeds_feed_a_record_of_up_to_two_blocks_whole(tmp_path, monkeypatch, before, size):
    """A record is fed whole when the block in which it begins and the one behind it hold its end: at offset 0, in the middle
    of a block, and ending exactly on a block's edge."""
    text = _small(before) + _record(1, size) + _small(1000)
    feeds, starts = _pieces(tmp_path, monkeypatch, text)
    big = int(np.searchsorted(starts, before))
    assert int(starts[big]) == before and int(starts[big + 1]) - before == size and before % BLOCK + size <= 2 * BLOCK
    got, n_records, holder = [], 0, None
    for piece, offsets in feeds:
        pos = len(b"".join(got))
        assert int(offsets[-1]) == piece.size and int(offsets[0]) == 0
        assert np.array_equal(offsets + np.uint64(pos), starts[n_records:n_records + offsets.size])
        if n_records <= big < n_records + offsets.size - 1:
            holder = piece.tobytes()[before - pos:before - pos + size]
        got.append(piece.tobytes())
        n_records += offsets.size - 1
    feeds.check()
    assert b"".join(got) == text and n_records == len(starts) - 1 and holder == text[before:before + size]


@pytest.mark.parametrize("before, size", REFUSED)
def test_record_feeds_refuse_a_record_that_two_blocks_do_not_hold(tmp_path, monkeypatch, before, size):
    """Refused: the carried tail and one further block do not hold the record's end.  The error names the record's 1-based
    number and the block size, and nothing of the record is yielded."""
    text = _small(before) + _record(2, size) + _small(1000)
    feeds, starts = _pieces(tmp_path, monkeypatch, text)
    big = int(np.searchsorted(starts, before))
    assert int(starts[big + 1]) - before == size and before % BLOCK + size > 2 * BLOCK
    got, n_records = [], 0
    with pytest.raises(ValueError) as exc:
        for piece, offsets in feeds:
            got.append(piece.tobytes())
            n_records += offsets.size - 1
    assert f"record {big + 1} is longer" in str(exc.value) and f"{BLOCK:,d} bytes" in str(exc.value) and "long.fq" in str(exc.value)
    assert n_records == big and b"".join(got) == text[:before]
