"""GPU: the Trimmer and the Corrector (kmer_trim.hip, kmer_correct.hip, kmer_trim.h) on feeds of the size and shape of real
ones, against trim_ref.runs and correct_ref.expected with exact equality of every field, the patched bytes, finish()'s totals
and the number of feeds.  The streams and their references are record_feed_inputs' (computed once per process);
test_record_feed_inputs_host.py asserts on the CPU that they reach what is named here.

The many-record stream, 70 000 records in one feed: 18 rounds of k_trim_scan (4096 = TRIM_SCAN_T * TRIM_SCAN_PER records
each: the carry `run` and the repeated wg_excl_sum on the same LDS words) and three passes of the capped grid (32 768 =
TRIM_MAX_WGS * TRIM_WAVES records each: a wave's second and third record in k_trim_count, k_trim_runs and k_correct_runs,
the ring and the CorrWalk of the record before; under the threshold trim_load_qual too).  The ragged feeds put a small feed
behind a large one and a large one behind a small one: the growth of the device buffers between feeds and the scan's `base`.
The long-line stream: lines 1 and 3 of up to 1000 bytes (the second and later rounds of trim_line_end, TRIM_ROUND = 256
bytes each), 63 .. 257 blanks in front of and behind the sequence (`first` and `last` of k_trim_count found in a late step or
round), reads of up to 4097 and of 40 000 bases (the ring of k_correct_runs wrapping many times), at k = 5, 9 and 13.

CPU time of the references (one core): about 16 s for the many-record stream with and without the threshold -- 5 s per
correct_ref.expected, 3 s per trim_ref.runs -- and about 13 s for the five long-line references, of which the three 64 MiB
tables of k = 13 take 1 s and their reference 2 s.  On the GPU every test is a few launches over at most 2 MB of text."""
import numpy as np
import pytest

import correct_ref
import record_feed_inputs as rfi
import trim_ref
from gpu_support import Device, lib

pytestmark = pytest.mark.gpu
T = rfi.T
FEEDS = (1, 4097, 3, 32769, 4096, 8193, 4095, 0, 16746)      # records per feed; 0: an empty feed, b"" and [0]
CUTTINGS = {"whole": None, "ragged": FEEDS}


def _pieces(fq, starts, sizes):
    """(the bytes, the offsets relative to them) of consecutive feeds of `sizes` records each; None: one feed."""
    R = len(starts) - 1
    sizes = [R] if sizes is None else list(sizes)
    assert sum(sizes) == R, (sum(sizes), R)
    buf = np.frombuffer(fq, dtype=np.uint8)
    lo = 0
    for n in sizes:
        a, b = int(starts[lo]), int(starts[lo + n])
        yield buf[a:b], starts[lo:lo + n + 1] - starts[lo]
        lo += n


def _by(per, R):
    return None if per is None else [min(per, R - lo) for lo in range(0, R, per)]


def _trim_all(t, fq, starts, sizes):
    parts = []
    for piece, offsets in _pieces(fq, starts, sizes):
        parts.append(t.feed(piece, offsets))
        assert all(v.size == offsets.size - 1 for v in parts[-1].values())
    return {name: np.concatenate([p[name] for p in parts]) for name in lib().TRIM_FIELDS}, len(parts)


def _correct_all(c, fq, starts, sizes):
    parts, texts = [], []
    for piece, offsets in _pieces(fq, starts, sizes):
        fields, text = c.feed(piece, offsets)
        assert all(v.size == offsets.size - 1 for v in fields.values()) and text.size == piece.size
        parts.append(fields)
        texts.append(text.tobytes())
    return {name: np.concatenate([p[name] for p in parts]) for name in lib().CORR_FIELDS}, b"".join(texts), len(parts)


def _where(a, b):
    """The first differing records, and where they lie among the scan rounds and the grid's passes."""
    at = np.flatnonzero(a != b)[:8]
    return at, at // rfi.SCAN_ROUND, at // rfi.STRIDE, a[at], b[at]


def _same_fields(got, want):
    for name in trim_ref.FIELDS:
        assert got[name].dtype == np.uint64 and got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape)
        assert np.array_equal(got[name], want[name]), (name,) + _where(got[name], want[name])


def _same(got, text, want):
    for name in correct_ref.FIELDS:
        assert got[name].dtype == np.uint64 and got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape)
        assert np.array_equal(got[name], want[name]), (name,) + _where(got[name], want[name])
    if text != want["patched"]:
        a, b = np.frombuffer(text, dtype=np.uint8), np.frombuffer(want["patched"], dtype=np.uint8)
        assert a.shape == b.shape, (a.shape, b.shape)
        at = np.flatnonzero(a != b)
        raise AssertionError(("patched bytes", at.size, at[:8], a[at[:8]], b[at[:8]]))


def _trim_totals(want):
    return {"n_records": int(want["seq_len"].size), "n_bases": int(want["n_bases"]), "n_covered": int(want["covered"].sum())}


# ------------------------------------------------------------------ the many-record stream: the Trimmer
@pytest.mark.parametrize("cutting", list(CUTTINGS))
def test_trimmer_many_records(gpu, cutting):
    fq, starts, want = rfi.many_stream(), rfi.many_starts(), rfi.many_trim()
    assert len(starts) - 1 == rfi.R_MANY
    with lib().Trimmer(0) as t:
        t.set_cover(want["bits"], want["n_bases"])
        got, feeds = _trim_all(t, fq, starts, CUTTINGS[cutting])
        _same_fields(got, want)                              # before finish(), whose guard would only say that a total differs
        fin, timings = t.finish(), t.timings()
    assert fin == _trim_totals(want)
    assert timings["trim_s"] > 0 and timings["feeds"] == feeds == (1 if cutting == "whole" else len(FEEDS))


def test_trimmer_many_records_device_form(gpu):
    fq, starts, want = rfi.many_stream(), rfi.many_starts(), rfi.many_trim()
    text = lib().DeviceBuffer(len(fq) + 1, 0)
    try:
        text.upload(np.frombuffer(b"x" + fq, dtype=np.uint8))            # the text at an odd address
        with lib().Trimmer(0) as t:
            t.set_cover(want["bits"], want["n_bases"])
            got = t.feed_device(text.ptr + 1, len(fq), starts)
            _same_fields(got, want)
            assert t.finish() == _trim_totals(want) and t.timings()["feeds"] == 1
        assert text.download()[1:].tobytes() == fq
    finally:
        text.free()


def test_trimmer_many_records_under_the_threshold(gpu):
    fq, starts, want = rfi.many_stream(T), rfi.many_starts(T), rfi.many_trim(T)
    assert 0 < want["n_bases"] < rfi.many_trim()["n_bases"]
    with lib().Trimmer(0) as t:
        t.set_cover(want["bits"], want["n_bases"], T)
        got, feeds = _trim_all(t, fq, starts, None)
        _same_fields(got, want)
        assert t.finish() == _trim_totals(want) and t.timings()["feeds"] == feeds == 1


# ------------------------------------------------------------------ the many-record stream: the Corrector
@pytest.mark.parametrize("cutting", list(CUTTINGS))
def test_corrector_many_records(gpu, cutting):
    fq, starts, want = rfi.many_stream(), rfi.many_starts(), rfi.many_correct()
    assert len(starts) - 1 == rfi.R_MANY
    with Device(rfi.many_tables()[0]) as dev, lib().Corrector(rfi.K_MANY, 0) as c:
        c.set_tables(dev.ptrs, 1, 255)
        c.set_cover(want["bits"], want["n_bases"], 0, 2)
        got, text, feeds = _correct_all(c, fq, starts, CUTTINGS[cutting])
        _same(got, text, want)
        fin, timings = c.finish(), c.timings()
    assert fin == correct_ref.totals(want)
    assert timings["correct_s"] > 0 and timings["feeds"] == feeds == (1 if cutting == "whole" else len(FEEDS))


def test_corrector_many_records_device_form(gpu):
    fq, starts, want = rfi.many_stream(), rfi.many_starts(), rfi.many_correct()
    text = lib().DeviceBuffer(len(fq) + 1, 0)
    out = lib().DeviceBuffer(len(fq) + 3, 0)
    try:
        text.upload(np.frombuffer(b"x" + fq, dtype=np.uint8))            # the text and its copy at odd addresses
        with Device(rfi.many_tables()[0]) as dev, lib().Corrector(rfi.K_MANY, 0) as c:
            c.set_tables(dev.ptrs, 1, 255)
            c.set_cover(want["bits"], want["n_bases"], 0, 2)
            got = c.feed_device(text.ptr + 1, len(fq), starts, out.ptr + 3)
            _same(got, out.download()[3:].tobytes(), want)
            assert c.finish() == correct_ref.totals(want) and c.timings()["feeds"] == 1
        assert text.download()[1:].tobytes() == fq                   # the text that is read is never written
    finally:
        text.free()
        out.free()


def test_corrector_many_records_under_the_threshold(gpu):
    fq, starts, want = rfi.many_stream(T), rfi.many_starts(T), rfi.many_correct(T)
    assert 0 < want["n_bases"] < rfi.many_correct()["n_bases"] and int(want["corrected"][rfi.STRIDE:].sum()) >= 100
    with Device(rfi.many_tables()[0]) as dev, lib().Corrector(rfi.K_MANY, 0) as c:
        c.set_tables(dev.ptrs, 1, 255)
        c.set_cover(want["bits"], want["n_bases"], T, 2)
        got, text, feeds = _correct_all(c, fq, starts, None)
        _same(got, text, want)
        assert c.finish() == correct_ref.totals(want) and c.timings()["feeds"] == feeds == 1


# ------------------------------------------------------------------ the long-line stream
def test_trimmer_long_lines(gpu):
    k = 5
    fq, starts, want = rfi.long_stream(k), rfi.long_starts(k), rfi.long_trim(k)
    R = len(starts) - 1
    for per in (None, 1, 7):
        with lib().Trimmer(0) as t:
            t.set_cover(want["bits"], want["n_bases"])
            got, feeds = _trim_all(t, fq, starts, _by(per, R))
            _same_fields(got, want)
            assert t.finish() == _trim_totals(want) and t.timings()["feeds"] == feeds == (1 if per is None else -(-R // per))


@pytest.mark.parametrize("k, M", [(5, 1), (5, 2), (5, None), (9, None), (13, None)])
def test_corrector_long_lines(gpu, k, M):
    fq, starts, want = rfi.long_stream(k), rfi.long_starts(k), rfi.long_correct(k, M)
    R = len(starts) - 1
    assert int(want["corrected"].sum()) > 0 and int(want["seq_len"].max()) == rfi.GIANT
    with Device(rfi.long_tables(k)[0]) as dev:
        for per in (None, 7):
            with lib().Corrector(k, 0) as c:
                c.set_tables(dev.ptrs, 1, 255)
                c.set_cover(want["bits"], want["n_bases"], 0, M)
                got, text, feeds = _correct_all(c, fq, starts, _by(per, R))
                _same(got, text, want)
                assert c.finish() == correct_ref.totals(want) and c.timings()["feeds"] == feeds == (1 if per is None else -(-R // per))
