"""GPU: every byte value through the record walkers.  Three readers must agree on what a valid base is: the FASTQ front end
and the parser that make the cover bits (QueryIndexer, fmt="fastq"), k_trim_count / k_trim_runs and k_correct_runs; where
one of them read a byte differently, every cover bit behind it would be shifted.  The texts are byte_inputs.placement_fastq
(every value in every line role, reads of up to 24 positions) with \\n and with \\r\\n, whole, and byte_inputs.walker_fastq
(every value at positions 10, 63, 64 and 130 of reads of 200, in line 2 and in line 4), without a threshold and with T = 53.
Per text: the lookup's n_bases and bits equal mask_ref's; the Trimmer and the Corrector take those very bits, report that
n_bases at finish() and equal trim_ref / correct_ref in every field; the Corrector's output differs from its input at the
reference's fix positions only; and the Trimmer equals trim_ref on bits from anywhere.
tests/test_seam_inputs_host.py asserts on the CPU what walker_fastq holds."""
import functools

import numpy as np
import pytest

import byte_inputs
import correct_inputs
import correct_ref
import fastq_qual_ref
import mask_ref
import trim_inputs
import trim_ref
from gpu_support import Device, lib, stream
from test_gpu_correct import _feed_all, _same
from test_gpu_trim import _feed_all as _feed_trim
from test_gpu_trim import _same_fields

pytestmark = pytest.mark.gpu
K, M = 5, 1
T = 53                                                       # the threshold byte of --min-qual 20 at offset 33
TEXTS = ("lf", "crlf", "walker")


@functools.lru_cache(maxsize=None)
def _tables():
    return correct_inputs.tables(K, 3, seed=805)


@functools.lru_cache(maxsize=None)
def _text(name: str, tq: int) -> bytes:
    if name == "walker":
        return byte_inputs.walker_fastq(_tables()[1])        # its own line 4: 50 .. 73 and every value
    fq = byte_inputs.placement_fastq(name == "crlf")
    return fastq_qual_ref.hand_qualities(fq, tq, seed=len(name)) if tq else fq


@functools.lru_cache(maxsize=None)
def _want(name: str, tq: int):
    """The reference of a text: computed once, shared by the tests, never changed."""
    return correct_ref.expected(_text(name, tq), K, _tables()[0], M=M, T=tq)


@pytest.fixture(scope="module")
def dev(gpu):
    with Device(_tables()[0]) as d:
        yield d


@pytest.mark.parametrize("name", TEXTS)
@pytest.mark.parametrize("tq", [0, T])
def test_lookup_trimmer_and_corrector_agree_on_every_byte(dev, name, tq):
    fq = _text(name, tq)
    want = _want(name, tq)
    starts = trim_ref.starts(fq)
    counts = {key: int(want[key].sum()) for key in ("candidates", "corrected", "ambiguous", "unfixable")}
    assert min(counts.values()) >= 100 and len(starts) - 1 >= 700, counts          # the comparison is not vacuous
    assert not tq or want["n_bases"] < _want(name, 0)["n_bases"]
    masked = mask_ref.expected(trim_ref.fasta_of(fq, tq), K, _tables()[0], 1, 255)
    with lib().QueryIndexer(K, device=0, fmt="fastq", min_qual_byte=tq) as q:       # reader 1: the front end and the parser
        q.set_tables(dev.ptrs, 1, 255)
        cover = stream(q, fq, cover=True, reset=False)
    assert cover["n_bases"] == masked["n_bases"] == want["n_bases"] and cover["fin"]["n_records"] == len(starts) - 1
    assert np.array_equal(cover["bits"], masked["bits"]) and np.array_equal(cover["bits"], want["bits"])
    geo = trim_ref.runs(fq, list(_tables()[0]), K, 1, 255, T=tq)
    for per in (None, 7):
        with lib().Trimmer(0) as t:                          # reader 2, on the lookup's own bits
            t.set_cover(cover["bits"], cover["n_bases"], tq)
            got = _feed_trim(t, fq, starts, per)
            fin = t.finish()
        _same_fields(got, geo)
        assert fin == {"n_records": len(starts) - 1, "n_bases": cover["n_bases"], "n_covered": int(geo["covered"].sum())}
        with lib().Corrector(K, 0) as c:                     # reader 3, on the same bits
            c.set_tables(dev.ptrs, 1, 255)
            c.set_cover(cover["bits"], cover["n_bases"], tq, M)
            fields, text = _feed_all(c, fq, starts, per)
            fin = c.finish()
        _same(fields, text, want)
        assert fin == correct_ref.totals(want) and fin["n_bases"] == cover["n_bases"]
        a, b = np.frombuffer(fq, dtype=np.uint8), np.frombuffer(text, dtype=np.uint8)
        fixed = want["pos2"][want["fix_record"].astype(np.int64)].astype(np.int64) + want["fix_pos"].astype(np.int64)
        assert np.array_equal(np.flatnonzero(a != b), fixed) and np.array_equal(b[fixed], want["fix_new"])


@pytest.mark.parametrize("name", TEXTS)
@pytest.mark.parametrize("tq", [0, T])
def test_trimmer_on_bits_from_anywhere_over_every_byte(gpu, name, tq):
    fq = _text(name, tq)
    starts = trim_ref.starts(fq)
    cover = trim_inputs.bits(_want(name, tq)["n_valid_bases"], seed=70 + tq)
    want = trim_ref.runs(fq, cover, T=tq)
    length = (want["trim_end"] - want["trim_start"]).astype(np.int64)
    assert int((want["covered"].astype(np.int64) > length).sum()) >= 50             # reads with more than one run
    for per in (None, 7):
        with lib().Trimmer(0) as t:
            t.set_cover(mask_ref.pack(cover), int(cover.size), tq)
            got = _feed_trim(t, fq, starts, per)
            fin = t.finish()
        _same_fields(got, want)
        assert fin == {"n_records": len(starts) - 1, "n_bases": int(cover.size), "n_covered": int(cover.sum())}
