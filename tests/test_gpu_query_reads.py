"""GPU: the query lookup on read-shaped input at k = 13, 15 and 17 -- the 32-bit instantiation with a smear over 12 and 14
bits and the 64-bit one, every option (bins, coordinates, spectrum, pairs) -- against the host restatements query_ref,
query_bins_ref, query_coords_ref, query_spectrum_ref and query_pairs_ref.  Every comparison is exact equality of integer
arrays.  The tables are counted on the GPU from query_ref.counted_sources and never leave HBM; the reference reads them as
SparseTables.  The inputs are query_ref's reads_case, rows_case and break_case; tests/test_query_host.py asserts on the CPU
that they reach what they are meant to reach (rows beyond every LDS accumulator, reads without a window, the break d bases
from the chunk boundary, hits that differ between the count windows and between the tables of a pair)."""
import contextlib
import functools
import types

import numpy as np
import pytest

import gpu_support as gs
import query_bins_ref
import query_coords_ref
import query_pairs_ref
import query_ref
import query_spectrum_ref
from fastq_qual_ref import mask_fastq_to_fasta
from gpu_support import binned, checked_pairs, checked_spectrum, lib, same, same_bins, same_coords, stream

pytestmark = pytest.mark.gpu
CHUNK = query_ref.CHUNK
WINDOWS = ((1, 255), (2, 254))
QACC_RECS, QSPEC_ROWS, QPAIR_ROWS = 128, 32, 64              # kmer_query.hip: the rows of a slot that are tallied in LDS


@contextlib.contextmanager
def _counted(k):
    """The counted tables of k (three, at k = 17 two of 16 GiB) in their indexers, and one QueryIndexer that every case
    streams through, with a reset between two streams."""
    lib = gs.lib()
    sources, sparse = query_ref.counted_case(k)
    with contextlib.ExitStack() as stack:
        ptrs = []
        for src in sources:
            ix = stack.enter_context(lib.Indexer(k, device=0))
            ix.feed(src)
            ix.finish()
            ptrs.append(ix.table_device_ptr())
        q = stack.enter_context(lib.QueryIndexer(k, device=0))
        yield types.SimpleNamespace(k=k, ptrs=ptrs, sparse=sparse, q=q)


@pytest.fixture(scope="module")
def k13(gpu):
    with _counted(13) as c:
        yield c


@pytest.fixture(scope="module")
def k15(gpu):
    with _counted(15) as c:
        yield c


@pytest.fixture(scope="module")
def k17(gpu):
    with _counted(17) as c:
        yield c


@pytest.fixture
def at_k(request, k):
    """The module's fixture of the case's k: built when the first case asks for it, kept to the end of the module."""
    return request.getfixturevalue(f"k{k}")


def only(*ks):
    return pytest.mark.parametrize("k", ks)


def _same_as_plain(got, plain, keys=("hits", "depth", "n_valid")):
    for key in keys:
        assert np.array_equal(got[key], plain[key]), key


@functools.lru_cache(maxsize=None)
def _spectrum_want(k, W=None):
    return query_spectrum_ref.expected(query_ref.reads_case(k), k, query_ref.counted_case(k)[1], W)


# ------------------------------------------------------------------ a. reads, every option ---------
@only(13, 15, 17)
@pytest.mark.parametrize("option", ["bins", "coords", "spectrum", "pairs"])
def test_reads_with_every_option(at_k, option):
    """3000 reads over seven chunks: several records in a thread's 16 windows, reads shorter than k, far more rows per
    slot than any LDS accumulator holds.  Each option against its reference under two count windows; hits, depth, n_valid
    and bin_first are those of the run with the option off, which is itself checked against query_ref."""
    k, q, tables = at_k.k, at_k.q, at_k.sparse
    text = query_ref.reads_case(k)
    for window in WINDOWS:
        q.set_tables(at_k.ptrs, *window)
        plain = stream(q, text)
        same(plain, query_ref.expected(text, k, tables, *window))
        assert plain["hits"].any(axis=0).all() and (plain["n_valid"] == 0).sum() > 3000 // 4
        if option == "bins":
            for W in (1, 3, 1000):
                want = query_bins_ref.expected(text, k, tables, *window, W)
                got = binned(q, text, W)             # (its record sums equal the unbinned run through the same indexer)
                same_bins(got, want)
                _same_as_plain(got, plain, ("hits", "depth"))
        elif option == "coords":
            want = query_coords_ref.expected(text, k, tables, *window, 3)
            got = stream(q, text, bins=3, coords=True)
            same_coords(got, want)
            off = binned(q, text, 3)
            _same_as_plain(got, off, ("bin_hits", "bin_depth", "bin_first"))
            assert np.array_equal(got["records"], off["records"])
        elif option == "spectrum":
            for W in (None, 3):
                got = checked_spectrum(q, text, window, _spectrum_want(k, W), W=W)      # (against the same stream with the option off)
                if W is None:
                    _same_as_plain(got, plain)
        else:
            for W in (None, 3):
                got = checked_pairs(q, text, query_pairs_ref.expected(text, k, tables, *window, W=W), W=W)
                assert got["shared"].any(axis=0).all()
                if W is None:
                    _same_as_plain(got, plain)


# ------------------------------------------------------------------ b. the same text cut into feeds
@only(17)
def test_reads_cut_into_feeds(at_k):
    k, q, tables = at_k.k, at_k.q, at_k.sparse
    text = query_ref.reads_case(k)
    hdr = text.index(b">", 3 * CHUNK + 100) + 2              # inside a header
    assert text[hdr - 2:hdr] == b">r" and text[hdr:hdr + 1].isdigit()
    cuts = sorted({7, 8, hdr, CHUNK, CHUNK + 5, 2 * CHUNK - 3, len(text) - 1})
    q.set_tables(at_k.ptrs, 1, 255)
    whole, cut = stream(q, text), stream(q, text, cuts=cuts)
    same(whole, query_ref.expected(text, k, tables, 1, 255))
    _same_as_plain(cut, whole)
    want = query_pairs_ref.expected(text, k, tables, 1, 255)
    whole, cut = checked_pairs(q, text, want), checked_pairs(q, text, want, cuts=cuts)
    assert np.array_equal(cut["shared"], whole["shared"])
    want = _spectrum_want(k)
    whole, cut = checked_spectrum(q, text, (1, 255), want), checked_spectrum(q, text, (1, 255), want, cuts=cuts)
    assert np.array_equal(cut["spectrum"], whole["spectrum"])


# ------------------------------------------------------------------ c. a feed that runs twice ------
@only(17)
@pytest.mark.parametrize("option", ["pairs", "spectrum"])
def test_retried_feed_counts_nothing_twice(at_k, option):
    """A fresh indexer, whose record array holds 4096 records, and 5000 reads in one feed: the squeeze backs out, the
    arrays grow and the feed runs again."""
    k, tables = at_k.k, at_k.sparse
    text = query_ref.reads_case(k, 5000)
    assert text.count(b">") == 5000 > 4096
    with lib().QueryIndexer(k, device=0) as q:
        q.set_tables(at_k.ptrs, 1, 255)
        if option == "pairs":
            want = query_pairs_ref.expected(text, k, tables, 1, 255)
            q.set_pairs(True)
        else:
            want = query_spectrum_ref.expected(text, k, tables)
            q.set_spectrum(True)
        q.feed(np.frombuffer(text, dtype=np.uint8))
        fin = q.finish()
        assert fin["n_records"] == 5000 and fin["num_kmers"] == int(want["n_valid"].sum())
        hits, depth = q.results(5000)
        exp = query_ref.expected(text, k, tables, 1, 255)
        assert np.array_equal(hits, exp["hits"]) and np.array_equal(depth, exp["depth"])
        if option == "pairs":
            assert np.array_equal(q.pairs(5000), want["shared"]) and want["shared"].any(axis=0).all()
        else:
            assert np.array_equal(q.spectrum(5000), want["spectrum"])


# ------------------------------------------------------------------ d. FASTQ -----------------------
@only(15, 17)
def test_fastq_reads_masked_and_not(at_k):
    k, tables = at_k.k, at_k.sparse
    fq = query_ref.reads_case(k, 3000, True)
    T = 33 + 20
    fasta, n_masked = mask_fastq_to_fasta(fq, T)
    with lib().QueryIndexer(k, device=0, fmt="fastq") as q:
        q.set_tables(at_k.ptrs, 1, 255)
        want = query_ref.expected(fq, k, tables, 1, 255, fmt="fastq")          # (through fastq_ref.fastq_to_fasta)
        assert len(want["records"]) == 3000 and (want["n_valid"] == 0).any()
        same(stream(q, fq), want)
        checked_pairs(q, fq, query_pairs_ref.expected(fq, k, tables, 1, 255, fmt="fastq"))
    with lib().QueryIndexer(k, device=0, fmt="fastq", min_qual_byte=T) as q:
        q.set_tables(at_k.ptrs, 1, 255)
        low = query_ref.expected(fasta, k, tables, 1, 255)
        assert n_masked > 1000 and 0 < int(low["n_valid"].sum()) < int(want["n_valid"].sum())     # some windows go, not all
        same(stream(q, fq), low)
        got = checked_pairs(q, fq, query_pairs_ref.expected(fasta, k, tables, 1, 255))
        assert got["shared"].any(axis=0).all()


# ------------------------------------------------------------------ e. row thresholds, 64-bit ------
def _rows(at_k, s, ragged, W, run):
    text, index = query_ref.rows_case(s, ragged, at_k.k)
    for window in WINDOWS:
        at_k.q.set_tables(at_k.ptrs, *window)
        run(at_k.q, text, index, window, W)


@only(17)
@pytest.mark.parametrize("W", [None, 5000])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("s", [QACC_RECS - 1, QACC_RECS, QACC_RECS + 1])
def test_long_record_at_the_last_lds_row_of_the_hits(at_k, s, ragged, W):
    """The 12 000-base record is row s of its slot: whole waves of it are summed and added by one lane, to LDS below row
    128 and to HBM from there on.  W = 5000: it has three rows, and every wave of it lies in one or two of them."""
    def run(q, text, index, window, W):
        if W is None:
            want = query_ref.expected(text, at_k.k, at_k.sparse, *window)
            assert want["hits"][index].all()
            same(stream(q, text), want)
        else:
            same_bins(binned(q, text, W), query_bins_ref.expected(text, at_k.k, at_k.sparse, *window, W))
    _rows(at_k, s, ragged, W, run)


@only(17)
@pytest.mark.parametrize("W", [None, 5000])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("s", [QSPEC_ROWS - 1, QSPEC_ROWS, QSPEC_ROWS + 1])
def test_long_record_at_the_last_lds_row_of_the_spectrum(at_k, s, ragged, W):
    def run(q, text, index, window, W):
        checked_spectrum(q, text, window, query_spectrum_ref.expected(text, at_k.k, at_k.sparse, W), W=W)
    _rows(at_k, s, ragged, W, run)


@only(17)
@pytest.mark.parametrize("W", [None, 5000])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("s", [QPAIR_ROWS - 1, QPAIR_ROWS, QPAIR_ROWS + 1])
def test_long_record_at_the_last_lds_row_of_the_pairs(at_k, s, ragged, W):
    def run(q, text, index, window, W):
        want = query_pairs_ref.expected(text, at_k.k, at_k.sparse, *window, W=W)
        assert want["shared"][-5:].any()                     # the long records share windows (their last rows, binned or not)
        checked_pairs(q, text, want, W=W)
    _rows(at_k, s, ragged, W, run)


# ------------------------------------------------------------------ f. a record break at a slot boundary
@only(13, 17)
def test_record_break_around_a_slot_boundary(at_k):
    """Record B begins d valid bases behind the second slot's first base, for every d in -k .. k: the restart lies in every
    bit the chunk start state and the first thread's smear can hold, on either side of the boundary.  Each text whole and
    cut at the chunk boundary; around d = 0 and at d = k - 1 also the pairs and bins of 7 windows."""
    k, q, tables = at_k.k, at_k.q, at_k.sparse
    q.set_tables(at_k.ptrs, 1, 255)
    for d in range(-k, k + 1):
        text = query_ref.break_case(k, d)
        want = query_ref.expected(text, k, tables, 1, 255)
        assert len(want["records"]) == 2 and want["hits"].all()
        whole, cut = stream(q, text), stream(q, text, cuts=[CHUNK])
        same(whole, want)
        _same_as_plain(cut, whole)
        if d in (-1, 0, 1, k - 1):
            pairs = query_pairs_ref.expected(text, k, tables, 1, 255)
            assert pairs["shared"].all()
            checked_pairs(q, text, pairs)
            checked_pairs(q, text, pairs, cuts=[CHUNK])
            want7 = query_bins_ref.expected(text, k, tables, 1, 255, 7)
            same_bins(binned(q, text, 7), want7)
            same_bins(binned(q, text, 7, cuts=[CHUNK]), want7)
