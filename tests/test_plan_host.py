"""Host-only checks of the partition-plan case table (tests/plan_ref.py): it covers every plan class that any legal
(k, slice count, feed <= 20 MiB) reaches, every case lies in the class it is listed under, and the texts built for the
cases put their windows where they claim.  pk_diag_plan_slice touches no GPU."""
import numpy as np
import pytest

import plan_ref
import slice_ref
from pykmer_amd import _lib


def _legal():
    """Every (k, n_slices) that pk_diag_plan_slice -- i.e. check_k, like pk_indexer_create_slice -- accepts."""
    out = []
    for k in range(1, 22, 2):
        for sb in range(0, 17):
            try:
                _lib.diag_plan_slice(k, 1 << sb, 1)
            except ValueError:
                continue
            out.append((k, 1 << sb))
    return out


def _feeds(k: int, n_slices: int):
    """1 byte, the cap, and both sides of every threshold of the plan: 8192 bytes per final bucket (byte counters below),
    one byte per 8 addresses (half-size buckets from there) and 1024 chunks (sampled layout from there).  The bucket counts
    themselves move with the feed (half-size buckets double them), so the thresholds are taken at both ends."""
    feeds = {1, plan_ref.FEED_CAP}
    for probe in (1, plan_ref.FEED_CAP):
        d = _lib.diag_plan_slice(k, n_slices, probe)
        for t in (8192 * d["B1"] * d["B2"], (1 << d["addr_bits"]) // 8, plan_ref.SAMPLED_FROM):
            feeds |= {t - 1, t}
    return sorted(n for n in feeds if 1 <= n <= plan_ref.FEED_CAP)


def test_the_diagnostic_refuses_what_the_indexer_refuses():
    legal = _legal()
    assert (1, 4) in legal and (7, 16384) in legal and (21, 256) in legal and (17, 1) in legal
    assert (1, 8) not in legal and (19, 1) not in legal and (19, 8) not in legal and (21, 128) not in legal
    for k, n_slices in ((2, 1), (23, 1 << 16), (15, 3), (15, 0), (15, 1 << 17), (19, 8)):
        with pytest.raises(ValueError):
            _lib.diag_plan_slice(k, n_slices, 1000)
    with pytest.raises(ValueError):
        _lib.diag_plan_slice(0, 1, 1000)


def test_every_plan_class_has_a_case():
    seen = {}
    for k, n_slices in _legal():
        for n in _feeds(k, n_slices):
            seen.setdefault(plan_ref.plan_class(_lib.diag_plan_slice(k, n_slices, n)), (k, n_slices, n))
    assert not any(c[2] == "none" for c in seen), "a legal plan that part_plan_check would refuse"
    missing = {c: at for c, at in seen.items() if c not in plan_ref.CASES}
    assert not missing, f"plan classes without a case in plan_ref.CASES (class: first (k, n_slices, n_bytes)): {missing}"
    extra = set(plan_ref.CASES) - set(seen)
    assert not extra, f"cases of classes that no legal plan reaches: {extra}"
    assert len(seen) >= 40


@pytest.mark.parametrize("cls", sorted(plan_ref.CASES, key=str), ids=lambda c: plan_ref.case_id(plan_ref.CASES[c]))
def test_case_lies_in_its_class_at_its_smallest_feed(cls):
    k, n_slices, s, n_bytes = plan_ref.CASES[cls]
    assert 0 <= s < n_slices and n_bytes % plan_ref.LINE == 0
    assert plan_ref.plan_class(_lib.diag_plan_slice(k, n_slices, n_bytes)) == cls
    # nothing larger than the class needs: one line less either leaves the class or is less than a text needs
    below = n_bytes - plan_ref.LINE
    assert below < plan_ref.text_floor(k) or plan_ref.plan_class(_lib.diag_plan_slice(k, n_slices, below)) != cls
    assert slice_prefix_is_ac(k, n_slices, s)
    sampled, kernel = cls[3], cls[4]
    if sampled:
        assert plan_ref.SAMPLED_FROM <= n_bytes < plan_ref.SAMPLED_FROM + plan_ref.LINE
    elif kernel == "bytes":
        assert n_bytes < (1 << 20)
    else:
        assert n_bytes <= (9 << 20)


def slice_prefix_is_ac(k, n_slices, s) -> bool:
    return n_slices == 1 or plan_ref.slice_prefix(k, n_slices, s)[:1] in (b"A", b"C")


@pytest.mark.parametrize("case", sorted(set(plan_ref.CASES.values())), ids=plan_ref.case_id)
def test_case_text_is_what_it_claims(case):
    """Exactly n_bytes, at least three records, one window in eight inside the tested slice and an address of it at 255
    (the oracle's count; tables of fewer than 16 addresses cannot hold the text's windows apart, the 255 is asked of them
    too), and the same hot unit under another seed."""
    k, n_slices, s, n_bytes = case
    text = plan_ref.focused_text(k, n_slices, s, n_bytes, 1)
    assert len(text) == n_bytes and text.endswith(b"\n") and b"\n\n" not in text
    e = slice_ref.Expect(text, k, n_slices)
    assert len(e.want["records"]) >= 3
    w = e.windows_per_slice()
    assert 8 * int(w[s]) >= int(w.sum()), (int(w[s]), int(w.sum()))
    addr, sat = e.slice(s)
    assert sat.size and int(sat.max()) == 255
    other = plan_ref.focused_text(k, n_slices, s, n_bytes, 2)
    hot = text.split(b"\n", 2)[1]
    assert other != text and other.split(b"\n", 2)[1] == hot and len(other) == n_bytes
    if s == 0:
        assert b"A" * 400 in text
    if 4 ** k // n_slices >= 16 and n_bytes > (1 << 20):
        assert addr.size >= min(4 ** k // n_slices, 1000)      # a large feed fills or spreads over the slice


@pytest.mark.parametrize("k", range(1, 18, 2))
def test_unsliced_plan_agrees_with_pk_diag_plan(k):
    for n in (1, 8191, 40_000, (1 << 20) + 1, plan_ref.SAMPLED_FROM, plan_ref.FEED_CAP, 200 << 20, 0):
        a, b = _lib.diag_plan_slice(k, 1, n), _lib.diag_plan(k, n)
        for f in ("capacity1", "capacity2", "B1", "B2", "fb_bits", "n_chunks", "fits_u32"):
            assert a[f] == b[f], (k, n, f)
        assert a["addr_bits"] == 2 * k and a["B1"] == 1 << a["b1"] and a["B2"] == 1 << a["b2"]
        assert a["variant"] == ("k17" if k == 17 else "k15" if k == 15 else "narrow")
