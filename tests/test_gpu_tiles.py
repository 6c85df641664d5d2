"""GPU: parser state and carried runs across the seams of the 1024-chunk scan tiles.

Per-chunk summaries are combined across a feed in tiles of SCAN_T = 1024 chunks, 16 MiB of text: kmer_count.hip reduces
every tile, scans the tile totals behind the stream carry and re-scans each tile behind its seed; k_query_scan walks the
slot counts 1024 at a time; k_fq_scan gives each of 1024 threads a run of ceil(n_chunks / 1024) chunks.  The texts of
inputs.tile_seam_fasta put the rare states -- a header line, a restart, pending blanks, a CR LF pair, a record boundary --
on byte 1024 * 16384 * t of a feed; tests/test_tile_inputs_host.py shows from the oracle alone that every such site
changes the answer when the state is lost there.  Everything is exact, against oracle / slice_ref / query_ref /
query_bins_ref / fastq_ref, and every test asserts that its feeds have more than 1024 chunks."""
import functools

import numpy as np
import pytest

import fastq_ref
import inputs
import oracle
import query_bins_ref
import query_ref
import slice_ref
from gpu_support import Device, binned, lib, query, same, same_bins
from slice_ref import N_SLICES, seam_slice

pytestmark = pytest.mark.gpu

CHUNK = 16384
SCAN_T = 1024
TILE = inputs.TILE
assert TILE == SCAN_T * CHUNK


def _chunks(n_bytes: int) -> int:
    return -(-n_bytes // CHUNK)


def _check_indexer(ix, data: bytes, k: int, tag):
    """finish() of a whole-table indexer that was fed `data` against oracle.count_fasta: totals, every record field, the
    table and the value histogram (gpu_support.check_against_oracle for feeds of our own cutting)."""
    fin = ix.finish()
    want = oracle.count_fasta(data, k)
    assert fin["num_kmers"] == want["num_kmers"], tag
    assert fin["total_bp"] == want["total_bp"], tag
    assert fin["n_records"] == len(want["records"]), tag
    recs = ix.records(fin["n_records"])
    for f in slice_ref.FIELDS:
        assert np.array_equal(recs[f], want["records"][f]), (tag, f, np.flatnonzero(recs[f] != want["records"][f])[:5])
    table = ix.table_to_host()
    assert np.array_equal(table, want["table"]), tag
    hist, _ = oracle.table_stats(want["table"])
    assert np.array_equal(fin["hist256"][1:], hist), tag
    assert int(fin["hist256"].sum()) == 4 ** k


# ------------------------------------------------------------------ 1. the indexer, one feed -------------------------
@pytest.mark.parametrize("case", range(6))
@pytest.mark.parametrize("k", [11, 15])
def test_indexer_tile_seams(gpu, k, case):
    """Up to four sites of inputs.tile_seam_fasta on bytes TILE, 2 TILE, ... of one feed: tile t's seed is the stream carry
    composed with the totals of tiles 0 .. t-1, and what it has to hold is the site's state."""
    sites_at = inputs.tile_cases(k)[case]
    text, sites = inputs.tile_seam_fasta(k, sites_at, seed=1000 * k + case)
    assert all(B % TILE == 0 and B // CHUNK >= SCAN_T for _, _, B in sites) and _chunks(len(text)) > max(B for _, _, B in sites) // CHUNK
    assert _chunks(len(text)) > SCAN_T
    with gpu.Indexer(k) as ix:
        ix.feed(text)
        assert ix.timings()["feeds"] == 1, "the text was meant to be one feed: its tile seams are the sites"
        _check_indexer(ix, text, k, (k, sites))


# ------------------------------------------------------------------ 2. the indexer, the second feed's seam -----------
@pytest.mark.parametrize("case", range(11))
@pytest.mark.parametrize("k", [11, 15])
def test_indexer_tile_seams_second_feed(gpu, k, case):
    """Two feeds of TILE + 3 CHUNK + 7 and TILE + 5 CHUNK bytes, a site on the tile seam of each: the second feed's seed is
    carry o tile 0 with the carry of a stream that is under way (records, offsets, a run and a line state of its own: the
    cut lies 7 bytes into a chunk).  One site of every kind lies on the second feed's seam."""
    sites_at = inputs.tile_second_feed_cases(k)[case]
    first, second = inputs.TILE_FEEDS
    text, sites = inputs.tile_seam_fasta(k, sites_at, seed=2000 * k + case, n_bytes=first + second, gap_chunks=2)
    feeds = [text[:first], text[first:]]
    assert [len(f) for f in feeds] == [first, second] and all(_chunks(len(f)) > SCAN_T for f in feeds)
    assert [B for _, _, B in sites] == [TILE, first + TILE] and all(B % TILE == 0 for B in (sites[0][2], sites[1][2] - first))
    with gpu.Indexer(k) as ix:
        for f in feeds:
            ix.feed(f)
        assert ix.timings()["feeds"] == 2
        _check_indexer(ix, text, k, (k, sites))


# ------------------------------------------------------------------ 3. deep windows ----------------------------------
@pytest.mark.parametrize("site", range(3))
@pytest.mark.parametrize("k", [19, 21])
def test_deep_tile_seam(gpu, k, site):
    """k = 19, 21 (test_gpu_deep's way): a carried run of k - 1 bases behind an N, one of more than k - 1, and a run whose
    newest bases lie three chunks back, at the tile seam.  The slice is the one of the window that crosses the seam and
    reaches furthest back, asserted from the oracle before anything runs."""
    n = N_SLICES[k]
    kind, d, B = inputs.tile_deep_sites(k)[site]
    text, sites = inputs.tile_seam_fasta(k, [(kind, d, B)], seed=3000 + 10 * k + site)
    assert B == TILE and _chunks(len(text)) > SCAN_T
    exp = slice_ref.Expect(text, k, n)
    assert slice_ref.crossing_windows(text, k, B) == k - 1
    s = seam_slice(exp, B)
    i = slice_ref.first_window_at(text, k, B)
    assert exp.slice_of(exp.kmers[i]) == s and exp.distinct_per_slice()[s] > 0
    with gpu.Indexer(k, slice_index=s, n_slices=n) as ix:
        ix.feed(text)
        assert ix.timings()["feeds"] == 1
        exp.check(ix, s, tag=(k, kind, d, s))


# ------------------------------------------------------------------ 4. query -----------------------------------------
@functools.lru_cache(maxsize=None)
def _query_text():
    k = 9
    text, sites = inputs.tile_seam_fasta(k, inputs.tile_query_sites(k), seed=4009, n_bytes=inputs.QUERY_TILE_BYTES, gap_chunks=1)
    return k, text, sites, tuple(query_ref.random_tables(k, 2, seed=4010))


def _query_text_checked():
    k, text, sites, tables = _query_text()
    cut = inputs.QUERY_TILE_CUT
    assert _chunks(len(text)) == 2 * SCAN_T + 5 and _chunks(cut) > SCAN_T and _chunks(len(text) - cut) > SCAN_T
    assert sorted(B // CHUNK for _, _, B in sites if B % CHUNK == 0) == [SCAN_T, 2 * SCAN_T]      # slots 1024 and 2048 of the text
    assert [(B - cut) // CHUNK for _, _, B in sites if (B - cut) % CHUNK == 0] == [SCAN_T]         # slot 1024 of the second feed
    return k, text, cut, tables


def test_query_more_than_1024_slots(gpu):
    """More than 2048 slots in one feed: k_query_scan walks the slot counts 1024 at a time, and slot_first of the slots
    from 1024 on hangs on the running total; the L1 / L2 tile seeds are not the identity.  Whole, and as two feeds of more
    than 1024 slots each (the second with windows and records before it); per record, and binned (W = 1 would take more
    than 1 GB of rows)."""
    k, text, cut, tables = _query_text_checked()
    with Device(tables) as dev:
        for mn, mx in ((1, 255), (2, 254)):
            want = query_ref.expected(text, k, tables, mn, mx)
            assert int(want["records"]["name_off"][0]) == 1 and int(want["records"]["name_off"][1]) > TILE  # a record across slot 1024
            assert len(want["records"]) > inputs.TINY_RECORDS and (want["n_valid"] == 0).any() and want["hits"].all(axis=1).any()
            same(query(text, k, dev.ptrs, mn, mx), want)
            same(query(text, k, dev.ptrs, mn, mx, cuts=[cut]), want)
        with lib().QueryIndexer(k, device=0) as q:
            q.set_tables(dev.ptrs, 1, 255)
            for W in (64, 4099):
                want = query_bins_ref.expected(text, k, tables, 1, 255, W)
                assert int(want["bin_first"][-1]) > len(text) // (2 * W)
                same_bins(binned(q, text, W), want)
                same_bins(binned(q, text, W, cuts=[cut]), want)


# ------------------------------------------------------------------ 5. FASTQ -----------------------------------------
@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("n_chunks", [1025, 2049, 3 * 1024 + 1])
def test_fastq_scan_runs(gpu, n_chunks, crlf):
    """k_fq_scan above 1024 chunks: per = 2 with the last 511 threads idle, per = 3, per = 4 with threads idle and a last
    run of one chunk.  One feed; the seams between the runs fall in lines of every role, five of them hand-placed
    (fastq_ref.seam_read_set).  Reference: fastq_ref.fastq_to_fasta, then the oracle; fastq_ref.stats."""
    k = 11
    fq, fa, names_at, placed = fastq_ref.seam_read_set(n_chunks, crlf, seed=n_chunks + crlf)
    per = -(-n_chunks // fastq_ref.SCAN_RUNS)
    assert _chunks(len(fq)) == n_chunks > SCAN_T and per == {1025: 2, 2049: 3, 3073: 4}[n_chunks]
    assert all(B % (per * CHUNK) == 0 for B in placed.values())
    assert fastq_ref.fastq_to_fasta(fq) == fa
    want = oracle.count_fasta(fa, k)
    assert len(want["records"]) == len(names_at)
    with lib().Indexer(k, device=0, fmt="fastq") as ix:
        ix.feed(fq)
        fin = ix.finish()
        assert ix.timings()["feeds"] == 1
        recs, stats, table = ix.records(fin["n_records"]), ix.fastq_stats(), ix.table_to_host()
    assert fin["num_kmers"] == want["num_kmers"] and fin["total_bp"] == want["total_bp"]
    assert fin["n_records"] == len(want["records"])
    for f in ("name_len", "seq_len", "n_valid_kmers"):
        assert np.array_equal(recs[f], want["records"][f]), (f, np.flatnonzero(recs[f] != want["records"][f])[:5])
    assert np.array_equal(recs["name_off"], names_at), np.flatnonzero(recs["name_off"] != names_at)[:5]   # names lie in the FASTQ
    assert np.array_equal(table, want["table"])
    assert np.array_equal(fin["hist256"][1:], oracle.table_stats(want["table"])[0])
    assert stats == fastq_ref.stats(fq)
