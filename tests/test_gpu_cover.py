"""GPU: the cover bits (kmer_cover.hip k_cover_scan / k_query_cover, pk_query_set_cover / pk_query_cover) against the host
restatement mask_ref, bit for bit.  tests/test_mask_host.py asserts on the CPU what the inputs are meant to hold: covered
and uncovered bases under every count window, a base whose only matching window ends in the next chunk or feed."""
import contextlib
import os
import tempfile

import numpy as np
import pytest

import gpu_support as gs
import mask_inputs as mi
import mask_ref
import oracle
import query_coords_inputs as qci
import query_ref
import synth
from gpu_support import Device, feed, lib, stream

pytestmark = pytest.mark.gpu
CHUNK = mi.CHUNK


def _cover(q, text: bytes, cuts=None):
    """One stream through an indexer whose tables are set; no reset behind it."""
    return stream(q, text, cover=True, cuts=cuts, reset=False)


def _same(got, want):
    bits, n_bases, fin = got["bits"], got["n_bases"], got["fin"]
    assert n_bases == want["n_bases"] and fin["n_records"] == want["n_records"] and fin["num_kmers"] == want["win_end"].size
    assert bits.dtype == np.uint8 and bits.shape == want["bits"].shape
    cover = mask_ref.unpack(bits, n_bases)
    assert np.array_equal(cover, want["cover"]), np.flatnonzero(cover != want["cover"])[:8]
    assert np.array_equal(bits, want["bits"])                # the bits behind the last base are zero


@pytest.fixture(scope="module", params=mi.KS)
def staged(gpu, request):
    """(k, BandTables, device pointers, one QueryIndexer) per k; at k = 15 two tables of 1 GiB."""
    k = request.param
    tabs = mi.band_tables(k)
    with contextlib.ExitStack() as stack:
        bufs = []
        for t in tabs:
            b = lib().DeviceBuffer(4 ** k, 0)
            stack.callback(b.free)
            dense = t.dense()
            b.upload(dense)
            del dense
            bufs.append(b)
        q = stack.enter_context(lib().QueryIndexer(k, device=0))
        yield k, tabs, [b.ptr for b in bufs], q


@pytest.mark.parametrize("name", [n for n, _ in mi.texts(5)])
def test_every_text_under_every_count_window(staged, name):
    k, tabs, ptrs, q = staged
    text = dict(mi.texts(k))[name]
    for window in mi.WINDOWS:
        want = mask_ref.expected(text, k, tabs, *window)
        q.reset()
        q.set_tables(ptrs, *window)
        _same(_cover(q, text), want)
    one = mask_ref.expected(text, k, tabs[:1], 1, 255)       # one table alone covers less than the two
    assert one["cover"].sum() < mask_ref.expected(text, k, tabs, 1, 255)["cover"].sum()
    q.reset()
    q.set_tables(ptrs[:1], 1, 255)
    _same(_cover(q, text), one)


def test_k17(gpu):
    """The 64-bit instantiation: another family member, then the indexed genome itself, against the genome's table."""
    k = 17
    text = qci.k17_text()
    genome = qci.k17_genomes()[0]
    sparse = [query_ref.SparseTable(oracle.kmer_list(genome, k))]
    lib = gs.lib()
    with lib.Indexer(k, device=0) as ix:
        ix.feed(genome)
        ix.finish()
        for window in ((1, 255), (2, 254)):
            want = mask_ref.expected(text, k, sparse, *window)
            assert 0 < want["cover"].sum() < want["n_bases"]
            with lib.QueryIndexer(k, device=0) as q:
                q.set_tables([ix.table_device_ptr()], *window)
                _same(_cover(q, text), want)


@pytest.mark.parametrize("which", ["around", "edge"])
def test_seams(gpu, which):
    """A one-record text of three chunks whose matching windows lie around the 16 KiB boundaries: fed whole, cut at every
    byte around a chunk seam (the bits reach back into the feed before) and cut one byte at a time over one line."""
    k, text = mi.SEAM_K, mi.seam_text()
    table = mi.seam_tables()[0 if which == "around" else 1]
    want = mask_ref.expected(text, k, [table], 1, 255)
    assert 0 < want["cover"].sum() < want["n_bases"]
    with Device([table]) as dev, lib().QueryIndexer(k, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        _same(_cover(q, text), want)
        for cut in mi.seam_cuts():
            q.reset()
            _same(_cover(q, text, [cut]), want)
        q.reset()
        _same(_cover(q, text, mi.line_cuts()), want)
        q.reset()
        _same(_cover(q, text, [CHUNK - 3, CHUNK + 2, 2 * CHUNK - 1, 2 * CHUNK + 1]), want)
        if which == "around":                                # counts of 2 around the even boundary only
            q.reset()
            q.set_tables(dev.ptrs, 2, 254)
            two = mask_ref.expected(text, k, [table], 2, 254)
            assert 0 < two["cover"].sum() < want["cover"].sum()
            _same(_cover(q, text, [2 * CHUNK - 4]), two)


def test_run_across_a_chunk_with_three_bases(gpu):
    """16 KiB of blank lines and line terminators in mid-sequence: the middle slot holds fewer than k - 1 bases of the run,
    and a matching window's bases span three slots."""
    k = mi.SEAM_K
    text, table = mi.hollow()
    want = mask_ref.expected(text, k, [table], 1, 255)
    with Device([table]) as dev, lib().QueryIndexer(k, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        _same(_cover(q, text), want)
        for cuts in ([CHUNK], [CHUNK + 2, 2 * CHUNK], [CHUNK - 1, CHUNK + 1, 2 * CHUNK - 5, 2 * CHUNK + 3]):
            q.reset()
            _same(_cover(q, text, cuts), want)


def test_more_chunks_than_the_scan_tile(gpu):
    k = mi.SEAM_K
    text, table = mi.long_text()
    want = mask_ref.expected(text, k, [table], 1, 255, fast=True)
    with Device([table]) as dev, lib().QueryIndexer(k, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        got = _cover(q, text)
        assert q.timings()["feeds"] == 1, "the text was meant to be one feed of 1026 chunks"
        _same(got, want)


def test_retry_in_the_second_feed_and_reset(gpu):
    """short_reads behind a small first feed: the second feed opens more records than the record array holds, its squeeze
    backs out (flag 2) and the feed runs again from the same base count.  Then the same indexer again after a reset, and a
    fresh one."""
    k = 5
    text = qci.short_reads()
    tabs = mi.band_tables(k)
    dense = [t.dense() for t in tabs]
    want = mask_ref.expected(text, k, tabs, 1, 255)
    assert want["n_records"] == 5000 > 4096 and 0 < want["cover"].sum() < want["n_bases"]
    with Device(dense) as dev:
        with lib().QueryIndexer(k, device=0) as q:
            q.set_tables(dev.ptrs, 1, 255)
            _same(_cover(q, text, [200]), want)
            q.reset()
            _same(_cover(q, text, [200]), want)
            q.reset()                                        # the bits of the stream before are gone
            other = qci.many_records(127)
            _same(_cover(q, other), mask_ref.expected(other, k, tabs, 1, 255))
            q.reset()
            with pytest.raises(lib().PkError):              # the bits are off after a reset
                feed(q, text)
                q.finish()
                q.cover(len(text))
        with lib().QueryIndexer(k, device=0) as q:
            q.set_tables(dev.ptrs, 1, 255)
            _same(_cover(q, text), want)


def test_seventeen_tables_and_three_staging_groups(gpu):
    """mask.cover_bits: 17 resident tables are two lookup launches within every feed; a budget of six tables stages the same
    17 in three groups whose bitmaps are OR-ed on the host.  Both give the bitmap of the reference over all 17."""
    from pykmer_amd import mask, merger, query
    k = 7
    rng = np.random.default_rng(1903)
    text = bytes(synth.family(3, 30_000)[0])
    kmers = np.unique(oracle.kmer_list(text, k))
    tables = []
    for i in range(17):                                      # every table holds a twentieth of the text's k-mers
        t = np.zeros(4 ** k, dtype=np.uint8)
        t[kmers[rng.random(kmers.size) < 0.05].astype(np.int64)] = 1 + i
        tables.append(t)
    want = mask_ref.expected(text, k, tables, 1, 255)
    last = mask_ref.expected(text, k, tables[:16], 1, 255)
    assert 0 < last["cover"].sum() < want["cover"].sum() < want["n_bases"]          # the seventeenth table adds bases
    with tempfile.TemporaryDirectory() as d, Device(tables) as dev:
        path = os.path.join(d, "q.fa")
        with open(path, "wb") as fh:
            fh.write(text)
        resident = [merger.ResidentTable(p, 4 ** k, 4 ** k, device=0) for p in dev.ptrs]
        for t in resident:
            t.kmer_len = k
        got = mask.cover_bits(path, resident, 1, 255, device=0)
        assert got["n_groups"] == 1 and got["n_bases"] == want["n_bases"] and np.array_equal(got["cover"], want["bits"])

        class _Host:                                         # a table that is staged: what stage() gets instead of a Header
            def __init__(self, i):
                self.i, self.kmer_len = i, k

        def stage(group, device):
            return query.Staged([dev.ptrs[t.i] for t in group])
        three = mask.cover_bits(path, [_Host(i) for i in range(17)], 1, 255, device=0, hbm_budget=6 * 4 ** k + 100, stage=stage)
        assert three["n_groups"] == 3 and np.array_equal(three["cover"], want["bits"]) and three["lookup_s"] > 0
