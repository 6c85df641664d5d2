"""The level-2 work order on the GPU: k_level1_finish ranks the level-1 buckets by size and deals them out to the XCD
classes, k_scatter2 walks them in that order (part_common.h: level2_rank / level2_position).  Whatever the order, the table
and its histogram equal the one-shot oracle's -- checked on texts whose bucket sizes are as uneven, as tied and as lopsided
as they get, on the two-level plan shapes of tests/plan_ref.py (exact and sampled layout, rooms from the slot sample and from
the record sample, a whole table and one slice of sixteen), and across the relayout retry, which computes the order anew.

Reference: slice_ref.Expect -- oracle.kmer_list over the whole text, np.unique, saturation at 255.  Integers, exact."""
import functools

import numpy as np
import pytest

import inputs
import plan_ref
import slice_ref

pytestmark = pytest.mark.gpu

# (k, n_slices, slice, feed bytes) and the plan class the feed must have: plan_ref.CASES
SHAPES = {
    "k15-exact": ("k15", 2, "final", False, "bytes", False),
    "k15-sampled": ("k15", 2, "final", True, "bytes", False),
    "k17-exact": ("k17", 2, "sample2", False, "bytes", False),
    "k15-16-slices": ("narrow_sliced", 2, "final", True, "half", False),
}
CONTENTS = ("ac_only", "uniform", "last_buckets")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _fit(head: bytes, seq: np.ndarray, n_bytes: int) -> bytes:
    """head + seq on 70-column lines, cut to exactly n_bytes with a line feed at the end."""
    body = plan_ref._wrap(seq)[:n_bytes - len(head)].copy()
    assert body.size == n_bytes - len(head), (body.size, n_bytes)
    if body[-2] == ord("\n"):                                # the cut fell right behind a line feed: no blank line
        body[-2] = ord("N")
    body[-1] = ord("\n")
    return head + body.tobytes()


@functools.lru_cache(maxsize=2)
def _text(content: str, k: int, n_slices: int, s: int, n_bytes: int) -> bytes:
    rng = np.random.default_rng([CONTENTS.index(content), k, n_slices])
    if content == "ac_only":                                 # canonical = the A/C word itself: address bits 0x0x0x..., a handful of level-1 buckets
        return _fit(b">a_and_c\n", ACGT[rng.integers(0, 2, size=n_bytes)], n_bytes)
    if content == "uniform":                                 # every bucket alike; in the small feeds most sizes tie
        return _fit(b">uniform\n", ACGT[rng.integers(0, 4, size=n_bytes)], n_bytes)
    # one window per unit: the slice's prefix, TTTT (a level-1 digit of all ones), random bases, AAAA (so that the other
    # strand begins with TTTT as well, or -- behind a slice prefix that begins with A -- is the larger word), N
    prefix = plan_ref.slice_prefix(k, n_slices, s)
    p = len(prefix)
    m = n_bytes // (k + 1) + 1
    u = np.empty((m, k + 1), dtype=np.uint8)
    u[:, :p] = np.frombuffer(prefix, dtype=np.uint8)
    u[:, p:p + 4] = ord("T")
    u[:, p + 4:k - 4] = ACGT[rng.integers(0, 4, size=(m, k - 8 - p))]
    u[:, k - 4:k] = ord("A")
    u[:, k] = ord("N")
    return _fit(b">last_buckets\n", u.reshape(-1), n_bytes)


def _level1_digits(exp, d, s):
    """The level-1 digits of the text's k-mers that lie in slice s."""
    mine = exp.kmers[(exp.kmers // np.uint64(exp.size)).astype(np.int64) == s] % np.uint64(exp.size)
    return (mine >> np.uint64(d["addr_bits"] - d["b1"])).astype(np.int64)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_two_level_tables_equal_the_oracle(gpu, shape, content):
    cls = SHAPES[shape]
    k, n_slices, s, n_bytes = plan_ref.CASES[cls]
    text = _text(content, k, n_slices, s, n_bytes)
    d = gpu.diag_plan_slice(k, n_slices, len(text))
    assert plan_ref.plan_class(d) == cls and d["B1"] >= 16
    exp = slice_ref.Expect(text, k, n_slices)
    digits = _level1_digits(exp, d, s)
    assert digits.size > 300, (shape, content, digits.size)      # the slice under test is busy
    used = np.unique(digits)
    if content == "ac_only":
        assert used.size <= 2 ** ((d["b1"] + 1) // 2), used      # every other bit of the digit is 0
    elif content == "last_buckets":
        assert used.min() >= d["B1"] - 2, used
    with gpu.Indexer(k, slice_index=s, n_slices=n_slices) as ix:
        ix.feed(text)
        exp.check(ix, s, full_table=True, tag=(shape, content))


@functools.lru_cache(maxsize=1)
def _skewed(stretch: int) -> bytes:
    data = inputs.skewed_fasta(16_503_000, 61, seed=68, stretch=stretch)
    assert len(data) >= 1024 * 16384                             # a sampled layout
    return data


@pytest.mark.parametrize("k,n_slices", [(15, 1), (17, 1), (15, 16)])
def test_the_order_is_computed_again_on_the_relayout_retry(gpu, k, n_slices):
    """The text that defeats the bucket sample, twice in a row on one indexer: both feeds overflow their sampled rooms and
    repeat the level-1 sort with exact sizes, so k_level1_finish runs twice per feed -- first returning at once on the
    raised flag with the order of the feed before (or none) still in the workspace, then on the retry."""
    data = _skewed(1024 if k == 17 else 2048)
    exp = slice_ref.Expect(data + data, k, n_slices)
    s = exp.busiest() if n_slices > 1 else 0
    with gpu.Indexer(k, slice_index=s, n_slices=n_slices) as ix:
        ix.feed(data)
        first = ix.timings()["relayouts"]
        assert first >= 1, "the skewed text was meant to overflow the sampled layout"
        ix.feed(data)
        assert ix.timings()["relayouts"] > first
        exp.check(ix, s, full_table=True, tag=(k, n_slices, s))
