"""GPU: the record walkers at the seams of their 64-position steps, on the enumerated streams of seam_inputs -- the Corrector
(kmer_correct.hip) on every (candidate position, distance to the run's end below, distance above) at the seams 64, 128 and
256, with every kind of byte that ends a run and with the read's own end, at k = 5 and 13, against correct_ref; the Trimmer
(kmer_trim.hip) on every cover pattern over the ten positions around the seams 64 and 256, with the ties that a run at the
read's start makes, against trim_ref.  Exact equality of every field, the patched bytes and the totals.
tests/test_seam_inputs_host.py asserts on the CPU that no enumerated case is missing from these streams.

CPU time of the references (one core of the GPU host): 0.1 .. 0.3 s per case and M at k = 5, 1.3 s at seam 64 to 2.7 s at
seam 256 per case and M at k = 13, 2 s and 3 s for the trimmer's two streams; about two and a half minutes for the file, of which
the GPU's part is a few launches over at most 3.6 MB of text per case."""
import pytest

import correct_ref
import mask_ref
import seam_inputs as si
import trim_ref
from gpu_support import Device, lib
from test_gpu_correct import _feed_all, _same
from test_gpu_trim import _feed_all as _feed_trim
from test_gpu_trim import _same_fields

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def staged(gpu):
    """The tables of both k in HBM, uploaded once: 1 KiB and 64 MiB."""
    with Device(si.case_tables(si.KS[0])[0]) as small, Device(si.case_tables(si.KS[1])[0]) as large:
        yield {si.KS[0]: small, si.KS[1]: large}


@pytest.mark.parametrize("k", si.KS)
@pytest.mark.parametrize("m", ["1", "default", "k"])
@pytest.mark.parametrize("seam, breaker, at_end", si.CASES)
def test_corrector_at_every_step_seam(staged, k, m, seam, breaker, at_end):
    fq, cover, cases = si.correct_case(k, seam, breaker, at_end)
    starts = trim_ref.starts(fq)
    tq = si.threshold_of(breaker)
    assert len(starts) - 1 == len(cases) == (2 * k + 2) * (k + 1) ** 2
    M = dict(zip(("1", "default", "k"), si.min_windows_of(k)))[m]
    want = si.correct_want(k, seam, breaker, at_end, M)
    assert int(want["candidates"].sum()) == sum(si.is_candidate(k, a, b) for _, a, b in cases) > 0
    for per in (None, 7):
        with lib().Corrector(k, 0) as c:
            c.set_tables(staged[k].ptrs, 1, 255)
            c.set_cover(mask_ref.pack(cover), int(cover.size), tq, M)
            got, text = _feed_all(c, fq, starts, per)
            fin = c.finish()
        _same(got, text, want)
        assert fin == correct_ref.totals(want), (M, per)


@pytest.mark.parametrize("seam", si.TRIM_SEAMS)
def test_trimmer_on_every_pattern_around_a_step_seam(gpu, seam):
    fq, cover, cases = si.trim_case(seam)
    want = si.trim_want(seam)
    starts = trim_ref.starts(fq)
    assert len(starts) - 1 == len(cases) >= 5 * (1 << si.WINDOW)
    for per in (None, 1000):
        with lib().Trimmer(0) as t:
            t.set_cover(mask_ref.pack(cover), int(cover.size))
            got = _feed_trim(t, fq, starts, per)
            fin = t.finish()
        _same_fields(got, want)
        assert fin == {"n_records": len(cases), "n_bases": int(cover.size), "n_covered": int(want["covered"].sum())}


@pytest.mark.parametrize("seam", si.TRIM_SEAMS)
def test_trimmer_with_a_position_that_holds_no_base_around_a_step_seam(gpu, seam):
    fq, cover, cases = si.trim_breakers(seam, seed=3990 + seam)
    want = trim_ref.runs(fq, cover)
    starts = trim_ref.starts(fq)
    for per in (None, 7):
        with lib().Trimmer(0) as t:
            t.set_cover(mask_ref.pack(cover), int(cover.size))
            got = _feed_trim(t, fq, starts, per)
            fin = t.finish()
        _same_fields(got, want)
        assert fin == {"n_records": len(cases), "n_bases": int(cover.size), "n_covered": int(want["covered"].sum())}
