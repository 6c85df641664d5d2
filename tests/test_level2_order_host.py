"""CPU: the order in which the level-2 sort walks the level-1 buckets (pk_diag_level2_order; the device's k_level1_finish
runs the same two functions of part_common.h).  Buckets are ranked by size, descending, ties by lower index; rank r goes to
round r // 8, and to XCD class r % 8 in even rounds, 7 - r % 8 in odd ones; position class * (B1 // 8) + round holds it."""
import numpy as np
import pytest

from pykmer_amd import _lib

B1S = (8, 16, 128, 512)


def falling(B1):
    """Sizes proportional to 2 (1 - (b + 1/2) / B1): what canonical k-mers (the smaller of two words) give the level-1
    buckets of a long random text, scaled to a million records per bucket on average."""
    b = np.arange(B1, dtype=np.float64)
    return np.round(2.0 * (1.0 - (b + 0.5) / B1) * 1e6).astype(np.uint32)


def profiles(B1):
    rng = np.random.default_rng(B1)
    one = np.zeros(B1, np.uint32)
    one[B1 // 2 + 1] = 12345
    few = rng.integers(0, 4, B1).astype(np.uint32)                       # many ties
    return {"equal": np.full(B1, 777, np.uint32), "one": one, "falling": falling(B1), "rising": falling(B1)[::-1].copy(),
            "ties": few, "random": rng.integers(0, 2 ** 32, B1, dtype=np.uint64).astype(np.uint32)}


def snake(c, rnd):
    return c if rnd % 2 == 0 else 7 - c


def ranked(sizes):
    """Bucket indices by size descending, ties by lower index."""
    return sorted(range(len(sizes)), key=lambda b: (-int(sizes[b]), b))


def class_loads(sizes, order):
    per = len(sizes) // 8
    return np.array([int(sizes[order[c * per:(c + 1) * per]].astype(np.uint64).sum()) for c in range(8)], dtype=np.float64)


@pytest.mark.parametrize("B1", B1S)
def test_order_is_a_permutation_with_every_rank_in_its_place(B1):
    per = B1 // 8
    for name, sizes in profiles(B1).items():
        order = _lib.diag_level2_order(sizes)
        assert order.dtype == np.uint32 and order.shape == (B1,)
        assert sorted(order.tolist()) == list(range(B1)), name
        by_rank = ranked(sizes)
        for c in range(8):
            for rnd in range(per):
                assert order[c * per + rnd] == by_rank[8 * rnd + snake(c, rnd)], (name, c, rnd)


@pytest.mark.parametrize("B1", B1S)
def test_ties_resolve_by_index(B1):
    per = B1 // 8
    order = _lib.diag_level2_order(np.full(B1, 5, np.uint32))            # all equal: rank = index
    for c in range(8):
        for rnd in range(per):
            assert order[c * per + rnd] == 8 * rnd + snake(c, rnd)
    zeros = np.zeros(B1, np.uint32)
    assert np.array_equal(_lib.diag_level2_order(zeros), order)
    one = zeros.copy()
    one[B1 - 1] = 1                                                      # the last bucket alone holds records: rank 0
    got = _lib.diag_level2_order(one)
    assert got[0] == B1 - 1
    rest = [b for b in ranked(one) if b != B1 - 1]
    assert rest == list(range(B1 - 1))
    assert got[per] == 0                                                 # rank 1 = the lowest index of the tie, class 1 round 0


def test_falling_sizes_are_balanced_at_128_buckets():
    sizes = falling(128)
    order = _lib.diag_level2_order(sizes)
    loads = class_loads(sizes, order)
    assert loads.max() / loads.mean() <= 1.01
    arithmetic = np.array([(a % 16) * 8 + a // 16 for a in range(128)])  # the order before: class = b % 8
    before = class_loads(sizes, arithmetic)
    assert 1.05 < before.max() / before.mean() < 1.06                    # 1.055


@pytest.mark.parametrize("B1", (0, 4, 12, 520, 1024))
def test_refuses_other_bucket_counts(B1):
    with pytest.raises(ValueError):
        _lib.diag_level2_order(np.ones(B1, np.uint32))
