"""Settled chunks: full 16 KiB chunks of plain sequence text that are not entered inside a header line.  The structure pass
of a counting feed squeezes them itself, under the assumption that they are entered in a live record behind a run of at
least k-1 bases and without pending blanks, and the squeeze pass completes them from the state they are really entered
with.  Every case here is the smallest text at which one of those state-dependent parts can go wrong; each is compared
with the one-shot oracle (records, totals, histogram, table), and each asserts that the library took the new path for
exactly the chunks a few lines of Python pick out of the same text."""
import functools

import numpy as np
import pytest

import oracle
import slice_ref
from inputs import record_overflows, record_starts

pytestmark = pytest.mark.gpu

CHUNK = 16384
WS = b" \t\n\v\f\r\x1c\x1d\x1e\x1f"                          # str.strip() whitespace, ASCII
DEEP_SLICES = 16                                             # k = 19: one of 16 address slices


# ------------------------------------------------------------------ the rule, in Python -------------------------------
def settled_chunks(text: bytes, begin: int, end: int) -> int:
    """Settled chunks of the feed text[begin:end] of the stream `text`: the chunk is full; it has no byte below 0x21 other
    than LF / CR and no '>'; its start lies outside header text.  (A line that starts inside such a chunk cannot be a
    header line: its '>' would be in the chunk.)"""
    n = 0
    for c0 in range(begin, end - CHUNK + 1, CHUNK):
        chunk = text[c0:c0 + CHUNK]
        if any((b < 0x21 and b not in (10, 13)) or b == 0x3e for b in set(chunk)):
            continue
        line_start = max(text.rfind(b"\n", 0, c0), text.rfind(b"\r", 0, c0)) + 1
        if text[line_start:c0].lstrip(WS).startswith(b">"):
            continue
        n += 1
    return n


# ------------------------------------------------------------------ texts ---------------------------------------------
def _body(rng, n_bytes: int, width: int = 61, eol: bytes = b"\n") -> bytearray:
    """n_bytes of random bases in lines of `width`."""
    n_lines = n_bytes // (width + len(eol)) + 1
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n_lines * width)].tobytes()
    return bytearray(eol.join(bases[i:i + width] for i in range(0, len(bases), width))[:n_bytes])


def _text(seed: int, n_chunks: float, head: bytes = b">r1 settled\n", **kw) -> bytearray:
    rng = np.random.default_rng(seed)
    return bytearray(head) + _body(rng, int(n_chunks * CHUNK) - len(head), **kw)


def _bases_back(text, at: int, n: int) -> int:
    """The position in front of `at` with exactly n base bytes between it and `at` (itself a base byte)."""
    p = at
    while True:
        p -= 1
        if text[p] in b"ACGT":
            if n == 0:
                return p
            n -= 1


def _pad_head(text: bytearray, head_len: int, delta: int) -> bytearray:
    """`delta` more bytes of header name: everything behind the header moves up by delta."""
    return text[:head_len - 1] + b"x" * delta + text[head_len - 1:]


def _carried_run_text(k: int, r: int) -> bytes:
    """An N with exactly r valid bases between it and the start of chunk 1; chunks 1 and 2 are settled, chunk 3 is partial."""
    t = _text(100 * k + r, 3.4)
    t[_bases_back(t, CHUNK, r)] = ord("N")
    return bytes(t)


# ------------------------------------------------------------------ the check -----------------------------------------
def _check(ix, text: bytes, k: int, deep, s: int, tag, deep_table: bool):
    if deep is not None:                                     # k = 19: one slice's value histogram; its 16 GiB image where asked for
        deep.check(ix, s, full_table=deep_table, tag=tag)
        return
    fin = ix.finish()
    want = _oracle(text, k)
    assert fin["num_kmers"] == want["num_kmers"], tag
    assert fin["total_bp"] == want["total_bp"], tag
    assert fin["n_records"] == len(want["records"]), tag
    recs = ix.records(fin["n_records"])
    for f in slice_ref.FIELDS:
        assert np.array_equal(recs[f], want["records"][f]), (tag, f, recs[f][:4], want["records"][f][:4])
    assert np.array_equal(ix.table_to_host(), want["table"]), tag
    hist, _ = oracle.table_stats(want["table"])
    assert np.array_equal(fin["hist256"][1:], hist), tag
    assert int(fin["hist256"].sum()) == 4 ** k


@functools.lru_cache(maxsize=4)
def _oracle(text: bytes, k: int):
    return oracle.count_fasta(text, k)


def _run(gpu, text: bytes, k: int, cuts=(), want_settled=None, tag=None, deep_table: bool = False):
    """Feeds text cut at `cuts`, checks the settled-chunk count of every feed against the Python rule (and the total
    against `want_settled`, the number the case was built for) and the result against the oracle.  k = 19 counts the
    busiest of 16 address slices; bringing its table to the host takes seconds, so one case (deep_table) does."""
    n_slices = DEEP_SLICES if k > 17 else 1
    deep = slice_ref.Expect(text, k, n_slices) if n_slices > 1 else None
    s = deep.busiest() if deep is not None else 0
    edges = [0, *cuts, len(text)]
    total = 0
    with gpu.Indexer(k, slice_index=s, n_slices=n_slices) as ix:
        for a, b in zip(edges, edges[1:]):
            ix.feed(text[a:b])
            want = settled_chunks(text, a, b)
            assert ix.settled_chunks() == want, (tag, a, b)
            total += want
        if want_settled is not None:
            assert total == want_settled, (tag, total)
        _check(ix, text, k, deep, s, tag, deep_table)


# ------------------------------------------------------------------ 1. carried run length -----------------------------
def _runs(k):
    return [(k, r) for r in range(k + 2)]


@pytest.mark.parametrize("k,r", _runs(5) + _runs(15) + _runs(19))
def test_carried_run(gpu, k, r):
    """r = 0: base 0 of the settled chunk restarts the run; r < k-1: its first k-1-r windows are void; r >= k-1: none is."""
    _run(gpu, _carried_run_text(k, r), k, want_settled=2, tag=(k, r), deep_table=r == k - 2)


# ------------------------------------------------------------------ 2. leading lanes ----------------------------------
@pytest.mark.parametrize("fill", [b"N", b"\n"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_leading_lanes(gpu, n, fill):
    """Chunk 1 begins with n Ns, or n bare LFs behind a run of 3 bases (every lane up to the first k-1 bases still
    depends on that run): more than one leading lane."""
    k = 15
    t = _text(7 * n + len(fill) + fill[0], 3.2, width=20000)            # no terminator of its own near the seam
    t[CHUNK:CHUNK + n] = fill * n
    t[_bases_back(t, CHUNK, 3)] = ord("N")
    _run(gpu, bytes(t), k, want_settled=2, tag=(n, fill))


@pytest.mark.parametrize("k", [5, 15])
def test_chunk_of_n_only(gpu, k):
    """A settled chunk without a single valid base: every lane leads, n_bases is 0."""
    t = _text(31, 3.2)
    for i in range(CHUNK, 2 * CHUNK):
        if t[i] != 10:
            t[i] = ord("N")
    _run(gpu, bytes(t), k, want_settled=2, tag=k)


# ------------------------------------------------------------------ 3. CR LF across the seam --------------------------
def test_crlf_across_the_seam(gpu):
    k = 15
    head = b">crlf\n"
    t = _text(41, 3.3, head=head, eol=b"\r\n")
    cr = t.rfind(b"\r", 0, CHUNK)
    t = _pad_head(t, len(head), CHUNK - 1 - cr)
    assert t[CHUNK - 1] == 13 and t[CHUNK] == 10
    _run(gpu, bytes(t), k, want_settled=2)


# ------------------------------------------------------------------ 4. pending blanks ---------------------------------
@pytest.mark.parametrize("k", [5, 15, 19])
@pytest.mark.parametrize("then", ["base", "terminator"])
def test_pending_blanks(gpu, k, then):
    """Chunk 1 ends in three blanks (it is not settled).  Chunk 2 is settled and begins with a base -- the blanks are
    interior: seq_len counts them and the run breaks -- or with the line's terminator: they are stripped."""
    head = b">pending\n"
    t = _text(51, 4.3, head=head)
    lf = t.rfind(b"\n", 0, 2 * CHUNK)
    t = _pad_head(t, len(head), 2 * CHUNK - lf + (20 if then == "base" else 0))
    assert t[2 * CHUNK + (20 if then == "base" else 0)] == 10
    t[2 * CHUNK - 3:2 * CHUNK] = b"   "
    _run(gpu, bytes(t), k, want_settled=2, tag=(k, then))


# ------------------------------------------------------------------ 5. text in front of the first header --------------
@pytest.mark.parametrize("k", [5, 15, 19])
def test_text_in_front_of_the_first_header(gpu, k):
    """Two plain chunks that belong to no record (settled, and dropped), a header, plain chunks of a record."""
    rng = np.random.default_rng(61)
    t = bytes(_body(rng, 2 * CHUNK + 100)) + b"\n>first\n" + bytes(_body(rng, 3 * CHUNK))
    _run(gpu, t, k, want_settled=4, tag=k)


# ------------------------------------------------------------------ 6. a header line longer than a chunk --------------
def test_long_header_line(gpu):
    """Chunk 1 is header text only and chunk 2 is entered inside the header line: neither is settled; 3 and 4 are."""
    k = 15
    rng = np.random.default_rng(71)
    t = b">" + b"h" * (2 * CHUNK + 300) + b"\n" + bytes(_body(rng, 3 * CHUNK))
    _run(gpu, t, k, want_settled=2)


# ------------------------------------------------------------------ 7. mixed content ----------------------------------
@pytest.mark.parametrize("k", [5, 15, 19])
def test_lower_case_and_iupac(gpu, k):
    """Lower-case bases and IUPAC letters inside settled chunks, alone and in runs; a partial last chunk."""
    rng = np.random.default_rng(81)
    t = _text(82, 4.6)
    letters = b"acgtacgtRYKMSWBDHVNn"
    for p in rng.integers(len(b">r1 settled\n"), len(t), size=1500):
        n = int(rng.integers(1, 4))
        for q in range(int(p), min(int(p) + n, len(t))):
            if t[q] != 10:
                t[q] = letters[int(rng.integers(len(letters)))]
    assert len(t) % CHUNK
    _run(gpu, bytes(t), k, want_settled=3, tag=k)


# ------------------------------------------------------------------ 8. feeds ------------------------------------------
@pytest.mark.parametrize("cuts", [(CHUNK,), (CHUNK, 2 * CHUNK), (CHUNK + 777,), (3001, 2 * CHUNK + 1)])
@pytest.mark.parametrize("k,r", [(15, 0), (15, 13), (15, 14), (5, 3), (19, 17)])
def test_settled_chunk_first_in_a_feed(gpu, k, r, cuts):
    """The text of test_carried_run in two and three feeds: a settled chunk that is the first of its feed takes its state
    from the carry; cuts at odd bytes move the chunk grid of the feeds behind them."""
    _run(gpu, _carried_run_text(k, r), k, cuts=cuts, tag=(k, r, cuts))


# ------------------------------------------------------------------ 9. record-array retry -----------------------------
def test_record_array_retry(gpu):
    """Feed 2 brings more records than the array holds, and long plain sequence behind them: its squeeze backs out and runs
    again over slots the structure pass wrote once."""
    k = 15
    rng = np.random.default_rng(91)
    first = bytes(_text(92, 2.5))
    reads = b"".join(b">s%d\n" % i + bytes(_body(rng, 24)) + b"\n" for i in range(5000))
    second = b"\n" + reads + b">long\n" + bytes(_body(rng, 4 * CHUNK + 500)) + b"\n"
    text = first + second
    _run(gpu, text, k, cuts=(len(first),), tag="retry")
    assert settled_chunks(text, len(first), len(text)) >= 3
    starts = record_starts(_oracle(text, k)["records"])
    assert record_overflows([len(first), len(second)], starts) == [False, True]


# ------------------------------------------------------------------ 10. sampled layout --------------------------------
def test_sampled_layout_over_settled_slots(gpu):
    """1100 chunks of plain sequence with a dozen records: the sampling launch and the sampled layout read slots that the
    structure pass wrote."""
    k = 15
    rng = np.random.default_rng(101)
    n_chunks = 1100
    per = n_chunks * CHUNK // 12
    text = b"".join(b">rec%d\n" % i + bytes(_body(rng, per - 8)) + b"\n" for i in range(12))
    assert gpu.diag_plan_slice(k, 1, len(text))["sample_stride"] > 1
    assert settled_chunks(text, 0, len(text)) >= n_chunks - 30
    _run(gpu, text, k, tag="sampled")
