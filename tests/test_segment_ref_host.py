"""CPU: the closed forms of segment_ref against the numpy yardsticks of the suite, on the layout of the tests past 2^32
at 1/2^20 of its size (blocks of 2^9 bytes, borders at 2^11 and 2^12), whose tables can be materialised; the folds;
and the coverage of the tables that meet every threshold."""
import numpy as np
import pytest

import combine_ref
import extract_ref
import oracle
import patterns_ref
import segment_ref as sr
from merge_ref import numpy_occgram, numpy_spectrum

FOLD, CLIP = 2 ** 12, 2 ** 11                                # the scaled 2^32 and 2^31


@pytest.fixture(scope="module")
def small():
    segs, n, at = sr.layout(**sr.SMALL)
    sparse, n2, at2 = sr.layout(sparse_present=sr.EXTRACT["P"], **sr.SMALL)
    assert (n, at) == (n2, at2) and n == FOLD + 4 + 37
    return segs, sparse, n, at


def _pair_of(tabs, mn, mx):
    """The upper-triangular pair matrix from the oracle's (N, N, 3) one: totals on the diagonal, shared tallies above."""
    m = oracle.gram(tabs, mn, mx)
    N = len(tabs)
    out = np.zeros((N, N), dtype=np.uint64)
    for i in range(N):
        out[i, i] = m[i, (i + 1) % N, 0]
        for j in range(i + 1, N):
            out[i, j] = m[i, j, 2]
    return out


def test_layout_is_what_the_tests_past_4gib_need():
    segs, n, at = sr.layout()
    assert n == 2 ** 32 + 2 ** 22 + 37 and 20 <= len(at) <= 28
    for x in (2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 32 - 1024, 2 ** 32 + 1023, n - 38, n - 1):
        assert x in at
    blocks = [sr.block_values(b) for b in range(9)]
    for i in range(sr.N_BASE):
        assert len({blocks[b][i] for b in range(8)}) == 8 and blocks[8][i] != blocks[0][i]
    flat = {v for b in blocks for v in b}
    assert {0, 1, 2, 3, 4, 5, 127, 128, 254, 255} <= flat
    assert sum(e - s for s, e, v in segs) == n and sum(1 for s, e, v in segs if e - s == 1) == len(at)


def test_fold_and_clip_by_hand():
    segs = [(0, 4, (1, 2)), (4, 5, (9, 9)), (5, 11, (3, 0))]
    a, b = sr.materialise(segs)
    fa, fb = sr.materialise(sr.fold(segs, 8))
    x = np.arange(11)
    assert np.array_equal(fa, a[x % 8]) and np.array_equal(fb, b[x % 8])
    ca, cb = sr.materialise(sr.clip(segs, 4))
    assert np.array_equal(ca, np.where(x < 4, a, 0)) and np.array_equal(cb, np.where(x < 4, b, 0))
    assert sr.check(sr.fold(segs, 8), 11) == (11, 2) and sr.check(sr.clip(segs, 4), 11) == (11, 2)
    assert sr.clip(segs, 11) == segs and sr.materialise(sr.fold(segs, 16))[0].tolist() == a.tolist()


@pytest.mark.parametrize("variant", ["true", "fold", "clip"])
def test_closed_forms_equal_the_yardsticks(small, variant):
    segs, sparse, n, _ = small
    cut = {"true": lambda s: s, "fold": lambda s: sr.fold(s, FOLD), "clip": lambda s: sr.clip(s, CLIP)}[variant]
    segs, sparse = cut(segs), cut(sparse)
    tabs = sr.materialise(segs)
    got = sr.results(segs, sparse)
    for kind, runs in (("pair", sr.PAIR_RUNS), ("sweep", [(N, sr.SWEEP_WINDOWS[:W]) for N, W in sr.SWEEP_RUNS])):
        for N, windows in runs:
            for w in windows:
                assert np.array_equal(got[kind, N, w], _pair_of([tabs[i] for i in sr.aliased(N)], *w)), (kind, N, w)
    assert np.array_equal(got["spectrum", 13], numpy_spectrum(tabs))
    for N in sr.OCC_RUNS:
        assert np.array_equal(got["occgram", N], numpy_occgram([tabs[i] for i in sr.aliased(N)])), N
    for N, windows in sr.PATTERN_RUNS:
        for w in windows:
            assert np.array_equal(got["patterns", N, w], patterns_ref.numpy_patterns([tabs[i] for i in sr.aliased(N)], *w)), (N, w)
    e = sr.EXTRACT
    P, cond = e["P"], (e["mn"], e["mx"], e["min_present"], e["max_absent"])
    five = [tabs[i] for i in e["tables"]]
    assert int(got["extract", "dense"][0]) == int(extract_ref.select_mask(five[:P], five[P:], *cond).sum())
    st = sr.materialise(sr.tables_of(sparse, e["tables"]))
    for first in (0, 2 ** 33 + 2048):
        addr, counts = sr.extract_rows(sr.tables_of(sparse, e["tables"]), P, *cond, first_addr=first)
        want_addr, want_counts = extract_ref.expected(st[:P], st[P:], *cond, first_addr=first)
        assert np.array_equal(addr, want_addr) and np.array_equal(counts, want_counts)
    for op in combine_ref.OPS:
        out, hist = sr.table(sr.tables_of(segs, e["tables"]), P, op, *cond)
        want = combine_ref.expected(five[:P], five[P:], op, *cond)
        assert np.array_equal(sr.materialise(out)[0], want), op
        assert np.array_equal(hist, combine_ref.hist256(want)) and np.array_equal(hist, got["table", op]), op
        assert np.array_equal(sr.window_bytes(out, n - 100, n), want[n - 100:]), op


def test_sparse_selection_is_sparse_and_reaches_past_the_border(small):
    _, sparse, n, at = small
    e = sr.EXTRACT
    addr, counts = sr.extract_rows(sr.tables_of(sparse, e["tables"]), e["P"], e["mn"], e["mx"], e["min_present"], e["max_absent"])
    assert 6 <= addr.size < len(at) and set(addr.tolist()) <= set(at)          # plants only, and not all of them
    assert (addr >= FOLD).sum() >= 2 and (addr < CLIP).sum() >= 2
    sub = sr.restrict(sr.tables_of(sparse, e["tables"]), FOLD + 16, n)            # a sub-slice that starts above the border
    a2, c2 = sr.extract_rows(sub, e["P"], e["mn"], e["mx"], e["min_present"], e["max_absent"], first_addr=FOLD + 16)
    keep = addr >= FOLD + 16
    assert keep.any() and np.array_equal(a2, addr[keep]) and np.array_equal(c2, counts[keep])


def test_folding_the_small_layout_changes_every_result(small):
    """What keeps the preconditions of the tests past 2^32 from being vacuous: at the scaled borders, too, a kernel that
    truncates its addresses gives another answer for every result, window and table."""
    segs, sparse, _, _ = small
    true = sr.results(segs, sparse)
    sr.assert_visible(true, sr.results(sr.fold(segs, FOLD), sr.fold(sparse, FOLD)), "fold")
    sr.assert_visible(true, sr.results(sr.clip(segs, CLIP), sr.clip(sparse, CLIP)), "clip")
    with pytest.raises(AssertionError):
        sr.assert_visible(true, sr.results(sr.fold(segs, 2 * FOLD), sr.fold(sparse, 2 * FOLD)), "no fold at all")


def test_full_size_layout_shows_a_truncation():
    """The same at full size, where nothing is materialised: the assertion the GPU tests repeat before they launch."""
    segs, n, _ = sr.layout()
    sparse, _, _ = sr.layout(sparse_present=sr.EXTRACT["P"])
    true = sr.results(segs, sparse)
    sr.assert_visible(true, sr.results(sr.fold(segs, 2 ** 32), sr.fold(sparse, 2 ** 32)), "fold")
    sr.assert_visible(true, sr.results(sr.clip(segs, 2 ** 31), sr.clip(sparse, 2 ** 31)), "clip")
    assert int(true["pair", 13, (1, 255)].max()) > 2 ** 32 - 2 ** 29          # tallies that a 32-bit counter could not hold either


# ------------------------------------------------------------------ the tables of the threshold tests
def test_threshold_tables_hold_every_value_at_every_offset():
    tabs = sr.threshold_tables(3, seed=11)
    assert len(tabs) == 3 and all(t.dtype == np.uint8 and t.size == 2 ** 19 for t in tabs)
    want = np.arange(256)
    for t in tabs:
        cols = np.sort(t.reshape(256, 2048), axis=0)         # column c = every address with x mod 2048 = c
        assert (cols == want[:, None]).all()
        for half in (0, 1024):                               # so every value at every x mod 16 in both KiB halves of a word group
            for r in range(16):
                assert (cols[:, half + r:half + 1024:16] == want[:, None]).all()
    a, b = tabs[0].reshape(256, 2048), tabs[1].reshape(256, 2048)
    assert (a != b).any(axis=0).all()                        # independent columns per table
    both = np.zeros((256, 256), dtype=bool)
    both[tabs[0], tabs[1]] = True
    for t in range(1, 256):                                  # a pair of tables meets every threshold from both sides
        assert both[t:, t:].any() and both[:t, t:].any() and both[t:, :t].any() and both[:t, :t].any()
    lists = sr.threshold_windows()
    assert [len(w) for w in lists] == [255, 255, 255] and len({w for ws in lists for w in ws}) == 762    # (1, 255), (255, 255) and (1, 1) twice
    assert all(1 <= mn <= mx <= 255 for ws in lists for mn, mx in ws)


def test_threshold_reference_equals_the_numpy_yardsticks():
    """threshold_ref on the CPU against oracle.gram, patterns_ref, extract_ref and combine_ref, at thresholds on both sides of 128."""
    import threshold_ref as tr
    tabs = [t[:2 ** 14] for t in sr.threshold_tables(5, seed=3)]
    T = tr.stack(tabs, "cpu")
    for mn, mx in ((1, 255), (1, 1), (127, 255), (128, 255), (1, 127), (1, 128), (129, 129), (200, 255), (255, 255), (3, 50)):
        m = tr.masks(T, mn, mx)
        assert np.array_equal(m.numpy(), np.stack([(t >= mn) & (t <= mx) for t in tabs]))
        assert np.array_equal(tr.pair(m), _pair_of(tabs, mn, mx)), (mn, mx)
        assert np.array_equal(tr.patterns(m[:3]), patterns_ref.numpy_patterns(tabs[:3], mn, mx)), (mn, mx)
        sel = tr.selection(m[:3], T[3:], 2, 1)
        assert np.array_equal(sel.numpy(), extract_ref.select_mask(tabs[:3], tabs[3:], mn, mx, 2, 1)), (mn, mx)
        for op in ("sum", "count"):
            want = combine_ref.expected(tabs[:3], tabs[3:], op, mn, mx, 2, 1)
            assert np.array_equal(tr.table(T[:3], m[:3], sel, op).numpy(), want), (mn, mx, op)
        none = tr.selection(m[:3], T[:0], 1, 0)
        assert np.array_equal(none.numpy(), extract_ref.select_mask(tabs[:3], [], mn, mx, 1, 0)), (mn, mx)
