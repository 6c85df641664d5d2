"""The launch tail of a feed on the GPU: the reset kernel (the tail becomes the empty stream's, the record array zero) and
the feed's one read-back, which brings the partition signals along with the stream totals.

Reuse: one indexer is fed, finished, reset and fed a different text; what it then reports is the second text's alone --
once with more records than the first text had (the record array grows behind the reset), once with fewer (record slots
the first text filled must read zero again: the squeeze adds into them).  FASTA and FASTQ indexers.

Feeds around the scan-tile size: texts of 1, 1023, 1024, 1025 and 2049 chunks at k = 7, a header line or an unwrapped
sequence line across every 1024-chunk seam, each as one feed and as the first and third of three consecutive feeds on one
indexer without a reset; the second has more records than the array holds, so that its squeeze backs out, the flag reaches
the host through the read-back and the squeeze is repeated and timed again.

Reference: oracle.count_fasta of the text (for FASTQ: of the FASTA text it stands for).  Integers, exact."""
import functools

import numpy as np
import pytest

import fastq_ref
import inputs
import oracle
from gpu_support import check_fastq_against_oracle
from inputs import record_overflows, record_starts

pytestmark = pytest.mark.gpu

FIELDS = ("name_off", "name_len", "seq_len", "n_valid_kmers")


def _same_as_oracle(ix, text, k, tag):
    fin = ix.finish()
    want = oracle.count_fasta(text, k)
    for key in ("num_kmers", "total_bp"):
        assert fin[key] == want[key], (tag, key, fin[key], want[key])
    assert fin["n_records"] == len(want["records"]), (tag, fin["n_records"], len(want["records"]))
    recs = ix.records(fin["n_records"])
    for f in FIELDS:
        assert np.array_equal(recs[f], want["records"][f]), (tag, f)
    assert np.array_equal(ix.table_to_host(), want["table"]), tag
    assert np.array_equal(fin["hist256"][1:], oracle.table_stats(want["table"])[0]), tag
    assert int(fin["hist256"].sum()) == 4 ** k, tag
    return want


@functools.lru_cache(maxsize=None)
def _fasta(many: bool) -> bytes:
    """10 001 records (more than a fresh indexer's 4096 slots), or 31."""
    if many:
        return inputs.record_dense_fasta(27 + 61 * 20_000, 2, seed=41)
    return inputs.record_dense_fasta(27 + 61 * 3_000, 100, seed=42)


@pytest.mark.parametrize("second_has_more", [True, False], ids=["more-records", "fewer-records"])
@pytest.mark.parametrize("k", [9, 13])
def test_fasta_indexer_reused_after_a_reset(gpu, k, second_has_more):
    first, second = _fasta(not second_has_more), _fasta(second_has_more)
    with gpu.Indexer(k) as ix:
        ix.feed(first)
        a = ix.finish()
        assert a["n_records"] == (31 if second_has_more else 10_001)
        ix.reset()
        assert ix.timings()["feeds"] == 0
        ix.feed(second)
        want = _same_as_oracle(ix, second, k, (k, second_has_more))
        assert len(want["records"]) == (10_001 if second_has_more else 31)
        assert ix.timings()["zero_s"] > 0                          # the reset's events bracket its kernel


@functools.lru_cache(maxsize=None)
def _fastq(many: bool) -> bytes:
    rng = np.random.default_rng(7 if many else 8)
    n_reads, length = (9_000, 80) if many else (40, 700)
    seqs = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n_reads, length))]
    qual = b"I" * length
    return b"".join(b"@r%d\n" % i + seqs[i].tobytes() + b"\n+\n" + qual + b"\n" for i in range(n_reads))


@pytest.mark.parametrize("second_has_more", [True, False], ids=["more-records", "fewer-records"])
def test_fastq_indexer_reused_after_a_reset(gpu, second_has_more):
    k = 9
    first, second = _fastq(not second_has_more), _fastq(second_has_more)
    with gpu.Indexer(k, fmt="fastq") as ix:
        ix.feed(first)
        a = ix.finish()
        assert a["n_records"] == (40 if second_has_more else 9_000)
        ix.reset()
        ix.feed(second)
        fin = ix.finish()
        got = dict(fin, records=ix.records(fin["n_records"]), stats=ix.fastq_stats(), table=ix.table_to_host())
    check_fastq_against_oracle(got, second, k)
    assert got["stats"] == fastq_ref.stats(second)


def test_reset_zeroes_a_record_array_of_more_than_one_grid_round(gpu):
    """140 001 records grow the array to about 420 000 slots of 32 bytes: more than the reset kernel's 2048 workgroups of 256
    lanes clear 16 bytes each in one round.  The text fed behind the reset has 31 records."""
    k = 9
    big = inputs.record_dense_fasta(27 + 61 * 280_000, 2, seed=46)
    with gpu.Indexer(k) as ix:
        ix.feed(big)
        assert ix.finish()["n_records"] == 140_001 > 2048 * 256 * 16 // 32 // 3
        ix.reset()
        ix.feed(_fasta(False))
        _same_as_oracle(ix, _fasta(False), k, "small text behind a large one")


# ------------------------------------------------------------------ feeds around the scan-tile size ----------------
CHUNK = 16384
HANDOVER_CHUNKS = (1, 1023, 1024, 1025, 2049)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _filler(rng, n: int) -> bytes:
    """Exactly n bytes of sequence lines, 60 columns but for the last one or two."""
    full, r = divmod(n, 61)
    if r == 1:                                                # a line feed alone would be a blank line
        full, r = full - 1, 62
    out = [inputs._lines(ACGT[rng.integers(0, 4, size=full * 60)], 60)] if full > 0 else []
    if r == 62:
        out += [ACGT[rng.integers(0, 4, size=30)].tobytes() + b"\n"] * 2
    elif r:
        out.append(ACGT[rng.integers(0, 4, size=r - 1)].tobytes() + b"\n")
    text = b"".join(out)
    assert len(text) == n, (len(text), n)
    return text


@functools.lru_cache(maxsize=2)
def _handover_text(n_chunks: int, content: str) -> bytes:
    """A text of n_chunks chunks (the last one 100 bytes short) that ends with a line feed.  Across every multiple of 1024
    chunks inside it -- where the summaries of one scan tile end and the next tile's begin -- lies a header line (content
    "header") or a sequence line of up to 20 000 bases (content "unwrapped"); a text without such a seam has the line
    across the start of its last chunk, a text of one chunk in its middle."""
    total = n_chunks * CHUNK - 100
    rng = np.random.default_rng([n_chunks, content == "header"])
    seams = list(range(inputs.TILE, total - 200, inputs.TILE)) or [(n_chunks - 1) * CHUNK or total // 2]
    parts, pos = [b">handover\n"], 10
    for j, B in enumerate(seams):
        if content == "header":
            line = b">seam_%d " % j + b"words and more words across the seam".ljust(50, b"x") + b"\n"
            start = B - 30
        else:
            n = min(20_000, total // 2)
            line = ACGT[rng.integers(0, 4, size=n)].tobytes() + b"\n"
            start = B - n // 2
        assert start - pos >= 200 and start < B < start + len(line) - 1
        parts += [_filler(rng, start - pos), line]
        pos = start + len(line)
    parts.append(_filler(rng, total - pos))
    text = b"".join(parts)
    assert len(text) == total and -(-total // CHUNK) == n_chunks and text.endswith(b"\n")
    return text


@functools.lru_cache(maxsize=1)
def _dense() -> bytes:
    return inputs.record_dense_fasta(27 + 61 * 60_000, 2, seed=45)                        # 30 001 records


@pytest.mark.parametrize("content", ["header", "unwrapped"])
@pytest.mark.parametrize("n_chunks", HANDOVER_CHUNKS)
def test_one_feed_around_the_scan_tile_size(gpu, n_chunks, content):
    k = 7
    text = _handover_text(n_chunks, content)
    with gpu.Indexer(k) as ix:
        ix.feed(text)
        _same_as_oracle(ix, text, k, (n_chunks, content))


@pytest.mark.parametrize("content", ["header", "unwrapped"])
@pytest.mark.parametrize("n_chunks", HANDOVER_CHUNKS)
def test_three_feeds_with_a_record_retry_in_the_middle(gpu, n_chunks, content):
    """The text, a record-dense text whose squeeze backs out and is repeated with a larger record array, and the text again,
    on one indexer without a reset: what a feed leaves behind for the next one -- the carried states, the signals, the
    events -- is armed again after a plain feed and after a retried one."""
    k = 7
    text = _handover_text(n_chunks, content)
    feeds = (text, _dense(), text)
    with gpu.Indexer(k) as ix:
        for f in feeds:
            ix.feed(f)
        t = ix.timings()
        assert t["feeds"] == 3 and t["squeeze_s"] > 0 and t["scan_s"] > 0
        want = _same_as_oracle(ix, b"".join(feeds), k, (n_chunks, content))
        assert record_overflows([len(f) for f in feeds], record_starts(want["records"])) == [False, True, False]
