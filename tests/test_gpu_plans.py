"""Every partition-plan class of the indexer on the GPU (tests/plan_ref.py: one case per class, checked against the plan
diagnostic by tests/test_plan_host.py), fresh and on top of an earlier feed, against the one-shot oracle of the whole text.

Reference: slice_ref.Expect -- oracle.kmer_list over both feeds in one piece, np.unique, saturation at 255, the slice by
address // slice size; the degenerate tables against oracle.count_fasta's whole table cut into slices.  Integers
throughout, every comparison exact."""
import functools
import time

import numpy as np
import pytest

import inputs
import oracle
import plan_ref
import slice_ref

pytestmark = pytest.mark.gpu

CLASSES = sorted(plan_ref.CASES, key=str)


@functools.lru_cache(maxsize=1)
def _case(case):
    """(text A, text A' -- same length, another seed, the same hot unit --, the oracle of A + A')."""
    k, n_slices, s, n_bytes = case
    a = plan_ref.focused_text(k, n_slices, s, n_bytes, 1)
    b = plan_ref.focused_text(k, n_slices, s, n_bytes, 2)
    return a, b, slice_ref.Expect(a + b, k, n_slices)


def _run_slice(gpu, cls, case, s, tested):
    k, n_slices, _, n_bytes = case
    a, b, expect = _case(case)
    with gpu.Indexer(k, slice_index=s, n_slices=n_slices) as ix:
        ix.feed(a)
        first = ix.timings()
        if tested and cls[4] == "bytes":                     # the hot unit wrapped a byte counter: the bucket was counted again
            assert first["buckets_recounted"] >= 1, first
        ix.feed(b)                                           # the same class on a table that is not fresh, bytes already at 255
        t = ix.timings()
        assert t["feeds"] == 2
        expect.check(ix, s, full_table=True, tag=(cls, case, s))
    return first, t


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: plan_ref.case_id(plan_ref.CASES[c]))
def test_plan_class_two_feeds_against_the_oracle(gpu, cls):
    case = plan_ref.CASES[cls]
    k, n_slices, s, n_bytes = case
    d = gpu.diag_plan_slice(k, n_slices, n_bytes)
    assert plan_ref.plan_class(d) == cls                     # the feeds below have exactly this length
    sampled = cls[3]
    t0 = time.perf_counter()
    first, t = _run_slice(gpu, cls, case, s, True)
    others = [] if sampled else [x for x in dict.fromkeys((0, n_slices - 1)) if x != s]
    for x in others:                                         # slice 0 (poly-A, address 0) and the last one (empty or nearly so)
        _run_slice(gpu, cls, case, x, False)
    print(f"\nplan-case {plan_ref.case_id(case)} class={cls} relayouts={t['relayouts']} buckets_recounted={first['buckets_recounted']}"
          f"+{t['buckets_recounted'] - first['buckets_recounted']} slices={[s] + others} wall={time.perf_counter() - t0:.2f}s")


# ------------------------------------------------------------------ tables of fewer than 16 addresses ---------------
DEGENERATE = [(1, 2), (1, 4), (3, 8), (3, 64), (5, 1024), (7, 16384)]


@functools.lru_cache(maxsize=None)
def _small_texts():
    import synth
    body, _ = synth.generate(77, 40_000, 3, pm_tandem=100, pm_dup=100, pm_ngap=30, pm_lower=50)
    return inputs.edge_fasta(), bytes(body)


@functools.lru_cache(maxsize=None)
def _whole_table(which: int, feeds: int, k: int):
    return oracle.count_fasta(_small_texts()[which] * feeds, k)["table"]


@pytest.mark.parametrize("k,n_slices", DEGENERATE)
def test_degenerate_tables_match_the_whole_table_cut_into_slices(gpu, k, n_slices):
    """Tables of 8, 2 and 1 addresses (n_slices = 4^k: one byte per table): every slice for k <= 3, the first two and the
    last otherwise; one feed on a fresh table, then two feeds after a reset."""
    size = 4 ** k // n_slices
    slices = range(n_slices) if k <= 3 else (0, 1, n_slices - 1)
    for s in slices:
        with gpu.Indexer(k, slice_index=s, n_slices=n_slices) as ix:
            for which, text in enumerate(_small_texts()):
                for feeds in (1, 2):
                    ix.reset()
                    for _ in range(feeds):
                        ix.feed(text)
                    fin = ix.finish()
                    want = _whole_table(which, feeds, k)[s * size:(s + 1) * size]
                    got = ix.table_to_host()
                    assert np.array_equal(got, want), (k, n_slices, s, which, feeds, got[:8], want[:8])
                    assert np.array_equal(fin["hist256"], np.bincount(want, minlength=256).astype(np.uint64)), (k, n_slices, s, which, feeds)
    if n_slices == 4 ** k:
        assert all(int(_whole_table(0, 1, k)[s]) > 0 for s in (0, 1))      # the one-byte tables of slices 0 and 1 are not empty


def test_one_byte_table_counts_the_issue_example(gpu):
    """k = 1 in four slices: `ACGT` holds A and T (address 0) and C and G (address 1); slices 2 and 3 stay empty."""
    for feeds in (1, 2):
        for s, want in enumerate((2, 2, 0, 0)):
            with gpu.Indexer(1, slice_index=s, n_slices=4) as ix:
                for _ in range(feeds):
                    ix.feed(b">x\nACGT\n")
                fin = ix.finish()
                assert int(ix.table_to_host()[0]) == want * feeds, (s, feeds)
                assert int(fin["hist256"][want * feeds]) == 1 and fin["num_kmers"] == 4 * feeds
