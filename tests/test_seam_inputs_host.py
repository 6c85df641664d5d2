"""CPU: the conditions that the streams of seam_inputs and byte_inputs.walker_fastq must meet for test_gpu_walker_seams.py
and test_gpu_walker_bytes.py to reach what they are there for, asserted from the generators and from correct_ref / trim_ref
alone.  No enumerated case may be missing: every (c, a, b) of every seam, breaker and variant is read back out of the
stream's own bytes and cover bits, not out of the generator's list; the reference calls a read a candidate exactly when
a + b - 1 >= k; every window count, every outcome class and every cover pattern occurs.  The constants the seams stand on
(TRIM_STEPS, TRIM_ROUND, CORR_RING) are read out of the sources, so that a change of them fails here and points at the seams
to move."""
import os

import numpy as np
import pytest

import byte_inputs
import correct_inputs
import correct_ref
import seam_inputs as si
import trim_ref
from fastq_ref import WS
from test_record_feed_inputs_host import _constant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("untried", "corrected", "ambiguous", "unfixable")
IS_LETTER = np.zeros(256, dtype=bool)
IS_LETTER[np.frombuffer(b"ACGTacgt", dtype=np.uint8)] = True


def test_the_seams_stand_on_the_kernels_constants():
    h = open(os.path.join(ROOT, "pykmer_amd", "csrc", "kmer_trim.h")).read()
    hip = open(os.path.join(ROOT, "pykmer_amd", "csrc", "kmer_correct.hip")).read()
    steps = int(_constant(h, "TRIM_STEPS"))
    assert _constant(h, "TRIM_ROUND") == "64u * TRIM_STEPS" and 64 * steps == si.SEAMS[-1] == si.TRIM_SEAMS[-1] == 256
    assert si.SEAMS[0] == si.TRIM_SEAMS[0] == 64 and si.SEAMS[1] % 64 == 0 and 64 < si.SEAMS[1] < 64 * steps      # a seam inside a round
    assert int(_constant(hip, "CORR_RING")) * 16 == 64 * steps            # the ring holds one round: seam 256 writes the word that seam 0 wrote
    assert max(si.KS) <= 17 and 2 * 17 < 64                               # a window reaches one step to either side at most


# ------------------------------------------------------------------ the corrector's cases
def _read_back(fq: bytes, cover: np.ndarray, tq: int):
    """[(c, a, b, seq_len, lead)] per read, from the text and the cover bits alone: the valid bases by the rule of README "Base
    quality" (a letter of ACGTacgt whose quality byte is not below the threshold), c the one valid base whose bit is zero,
    a and b the distances to the nearest position without a valid base (the read's ends count), FAR beyond k."""
    out, g = [], 0
    rows = fq.split(b"\n")                                   # these streams hold no \r, and no \n but the line ends
    assert rows[-1] == b"" and len(rows) % 4 == 1 and b"\r" not in fq
    for line1, line2, line3, line4 in zip(*(rows[j:-1:4] for j in range(4))):
        assert line1.startswith(b"@") and line3 == b"+" and len(line4) == len(line2)
        lead = len(line2) - len(line2.lstrip(WS))
        seq = np.frombuffer(line2.strip(WS), dtype=np.uint8)
        qual = np.frombuffer(line4, dtype=np.uint8)[lead:lead + seq.size]
        valid = IS_LETTER[seq] & ((qual >= tq) if tq else True)
        bits = cover[g:g + int(valid.sum())]
        g += int(valid.sum())
        zero = np.flatnonzero(valid)[~bits]
        assert zero.size == 1, "one uncovered base per read"
        c = int(zero[0])
        bad = np.concatenate([[-1], np.flatnonzero(~valid), [seq.size]])
        out.append((c, c - int(bad[bad < c].max()), int(bad[bad > c].min()) - c, int(seq.size), lead))
    assert g == cover.size
    return out


@pytest.mark.parametrize("k", si.KS)
def test_every_triple_of_every_seam_breaker_and_variant_is_in_the_stream(k):
    for seam, breaker, at_end in si.CASES:
        fq, cover, cases = si.correct_case(k, seam, breaker, at_end)
        want = si.triples(k, seam)
        assert cases == want and len(want) == len(set(want)) == (2 * k + 2) * (k + 1) ** 2
        got = _read_back(fq, cover, si.threshold_of(breaker))
        far = lambda d: d if d <= k else si.FAR               # noqa: E731
        assert [(c, far(a), far(b)) for c, a, b, _, _ in got] == want, (seam, breaker, at_end)
        assert {c for c, _, _ in want} == set(range(seam - k - 1, seam + k + 1))
        lengths = {n for _, _, _, n, _ in got}
        if at_end:
            assert all(n == c + b for c, a, b, n, _ in got) and seam in lengths and {seam - 1, seam + 1} <= lengths     # the run ends with the read
        else:
            assert lengths == {seam + 64} and all(b > k for (_, _, b, _, _), (_, _, fb) in zip(got, want) if fb == si.FAR)
        assert {lead for *_, lead in got} == {0, 1, 2, 3}
        if breaker == "other":
            held = np.frombuffer(fq, dtype=np.uint8)
            assert (held == 0x00).any() and (held == 0xC3).any()


def _check_case(k, seam, breaker, at_end, M):
    fq, cover, cases = si.correct_case(k, seam, breaker, at_end)
    want = si.correct_want(k, seam, breaker, at_end, M)
    is_cand = np.array([si.is_candidate(k, a, b) for _, a, b in cases])
    n_win = np.array([si.windows(k, a, b) for _, a, b in cases])
    assert np.array_equal(want["candidates"], is_cand.astype(np.uint64)), (k, seam, breaker, at_end)
    assert set(n_win[is_cand].tolist()) == set(range(1, k + 1))            # every window count
    m = correct_ref.default_min_windows(k) if M is None else M
    assert np.array_equal(want["untried"], (is_cand & (n_win < m)).astype(np.uint64))
    assert int(want["untried"].sum()) > 0 or m == 1
    assert want["n_bases"] == cover.size and not want["cover"].all()
    return {name: int(want[name].sum()) for name in ("candidates",) + CLASSES}


@pytest.mark.parametrize("seam", si.SEAMS)
def test_the_reference_at_k5_candidates_windows_and_classes(seam):
    k = 5
    held = np.count_nonzero(si.case_tables(k)[0][0]) / (4 ** k // 2)
    assert 0.4 < held < 0.6, held
    for breaker in si.BREAKERS:
        for at_end in (False, True):
            for M in si.min_windows_of(k):
                counts = _check_case(k, seam, breaker, at_end, M)
                print(k, seam, breaker, at_end, M, counts)
                assert min(counts[name] for name in CLASSES[1:]) > 0, counts       # tried ones of every class, at M = k too


def test_the_reference_at_k13_puts_nearly_every_tried_base_back():
    k = 13
    for case, M in (((64, "N", False), 1), ((64, "N", False), None), ((64, "qual", True), k)):
        counts = _check_case(k, *case, M)
        print(k, case, M, counts)
        tried = counts["candidates"] - counts["untried"]
        assert tried >= 100 and counts["corrected"] >= 0.9 * tried, counts
    assert si.min_windows_of(k) == (1, None, k) and len(si.CASES) == len(set(si.CASES)) == 24       # every case runs at every M


# ------------------------------------------------------------------ the trimmer's cases
@pytest.mark.parametrize("seam", si.TRIM_SEAMS)
def test_trim_cases_hold_every_pattern_and_the_ties_across_the_seam(seam):
    fq, cover, cases = si.trim_case(seam)
    want = si.trim_want(seam)
    lo = seam - si.WINDOW // 2
    n_valid = want["n_valid_bases"].astype(np.int64)
    assert np.array_equal(n_valid, want["seq_len"].astype(np.int64))       # every base valid: a bit per position
    first = np.concatenate([[0], np.cumsum(n_valid)])
    weights = 1 << np.arange(si.WINDOW)
    seen = {}
    for r, (pattern, head, tail) in enumerate(cases):
        bits = cover[first[r]:first[r + 1]]
        assert int((bits[lo:lo + si.WINDOW] * weights).sum()) == pattern and int(bits.sum()) == bin(pattern).count("1") + head + tail
        assert bits[:head].all() and bits[seam + 64:].sum() == tail and (tail == 0 or not bits[seam + si.WINDOW // 2:seam + 64].any())
        seen.setdefault(pattern, set()).add((head, tail))
    assert set(seen) == set(range(1 << si.WINDOW))                         # no pattern is missing
    for pattern, with_ in seen.items():
        heads = {h for h, t in with_ if h}
        assert {(0, 0), (0, si.TAIL_RUN)} <= with_ and set(si.near_ties(pattern)) <= heads | {0}
        assert seam != 64 or heads == set(si.TIE_RUNS)
    s, e = want["trim_start"].astype(np.int64), want["trim_end"].astype(np.int64)
    crossing = (s < seam) & (e > seam)
    assert int(crossing.sum()) >= 500 and {int(v) for v in (e - s)[crossing]} == set(range(2, si.WINDOW + 1))
    # an earlier run of equal length wins over one that crosses the seam, and the crossing one wins when it is one longer
    tie = loses = grows = 0
    for r, (pattern, head, tail) in enumerate(cases):
        across = [(lo + j, n) for j, n in si.pattern_runs(pattern) if lo + j < seam < lo + j + n]
        if not head or not across:
            continue
        (at, n), = across
        longest = max(m for _, m in si.pattern_runs(pattern))
        if n == longest == head:
            tie += 1
            assert (s[r], e[r]) == (0, head)
            grows += at + n - seam >= 1 and seam - at < head       # the open run becomes as long as the best only behind the seam
        if n == longest == head + 1 and not any(m == n and lo + j < at for j, m in si.pattern_runs(pattern)):
            loses += 1
            assert (s[r], e[r]) == (at, at + n)
    assert min(tie, loses, grows) >= 100, (tie, loses, grows)
    # behind a step without a set bit the run at seam + 64 stands alone, whatever was open at the seam: the patterns that end
    # in a run up to position seam - 1 and hold nothing behind it
    half = si.WINDOW // 2
    open_then_tail = [r for r, (pattern, head, tail) in enumerate(cases) if tail and (pattern >> (half - 1)) == 1]
    assert len(open_then_tail) == 1 << (half - 1)
    for r in open_then_tail:
        before = max(n for _, n in si.pattern_runs(cases[r][0]))
        assert e[r] - s[r] == max(before, si.TAIL_RUN) and (s[r] == seam + 64) == (before < si.TAIL_RUN)
    assert sum(int(s[r] == seam + 64) for r in open_then_tail) >= 4


@pytest.mark.parametrize("seam", si.TRIM_SEAMS)
def test_trim_breakers_put_an_invalid_byte_on_every_position_around_the_seam(seam):
    fq, cover, cases = si.trim_breakers(seam, seed=3990 + seam)
    want = trim_ref.runs(fq, cover)
    lo = seam - si.WINDOW // 2
    assert {(p, byte) for p, byte in cases} == {(p, byte) for p in range(lo, lo + si.WINDOW) for byte in si.TRIM_BREAKS}
    assert (want["seq_len"] == 2 * seam).all() and (want["n_valid_bases"] == 2 * seam - 1).all()
    s, e = want["trim_start"].astype(np.int64), want["trim_end"].astype(np.int64)
    p = np.array([c[0] for c in cases])
    assert ((e <= p) | (s > p)).all()                                      # no kept run holds the position
    assert int(((s == p + 1) & (p + 1 >= seam - 1)).sum()) >= 10 and int(((e == p) & (p <= seam + 1)).sum()) >= 10   # runs that begin and end at the seam


# ------------------------------------------------------------------ sixteen tables
def test_sixteen_tables_every_one_of_them_matters():
    k = 5
    tabs, _ = si.sixteen_tables(k)
    fq = si.sixteen_stream(k)
    assert len(tabs) == si.N_SIXTEEN and all(np.count_nonzero(t) >= 5 for t in tabs)
    union = np.zeros(4 ** k, dtype=np.int64)
    for t in tabs:
        union += t != 0
    assert union.max() == 1 and 0.4 < (union != 0).sum() / (4 ** k // 2) < 0.6          # an address lies in one table only
    want, less = correct_ref.expected(fq, k, tabs, M=1), correct_ref.expected(fq, k, tabs[:-1], M=1)
    counts = {name: int(want[name].sum()) for name in CLASSES}
    print(counts)
    assert min(counts[name] for name in CLASSES[1:]) >= 10, counts
    assert want["patched"] != less["patched"] and not np.array_equal(want["cover"], less["cover"])
    assert int(_constant(open(os.path.join(ROOT, "pykmer_amd", "csrc", "pk_kernels.h")).read(), "QUERY_MAX_TABLES")) == si.N_SIXTEEN


# ------------------------------------------------------------------ every byte value at the walkers' positions
def test_walker_fastq_holds_every_value_on_both_sides_of_a_step_seam():
    tabs, genome = correct_inputs.tables(5, 3, seed=805)
    fq = byte_inputs.walker_fastq(genome)
    recs = trim_ref.record_lines(fq)
    assert len(recs) == 3 * 254
    at2 = {p: set() for p in byte_inputs.WALKER_AT}
    at4 = {p: set() for p in byte_inputs.WALKER_AT}
    for i, (l1, l2, l3, l4, end) in enumerate(recs):
        assert l2[1] - l2[0] == l4[1] - l4[0] == byte_inputs.WALKER_LEN
        for p in ((10, 64), (63, 130), ())[i % 3]:
            at2[p].add(fq[l2[0] + p])
        for p in byte_inputs.WALKER_AT if i % 3 == 2 else ():
            at4[p].add(fq[l4[0] + p])
    every = set(range(256)) - {10, 13}
    assert all(v == every for v in at2.values()) and all(v == every for v in at4.values())
    for T in (0, 53):
        want = correct_ref.expected(fq, 5, tabs, M=1, T=T)
        counts = {name: int(want[name].sum()) for name in ("candidates",) + CLASSES}
        print(T, counts)
        assert min(counts[name] for name in CLASSES[1:]) >= 50, (T, counts)
        fp = want["fix_pos"].astype(np.int64)
        for p in byte_inputs.WALKER_AT:                                    # corrected bases within k - 1 of every placement
            assert int((np.abs(fp - p) < 5).sum()) >= 20, (T, p)
