"""GPU: base coordinates of binned query hits (pk_query_set_coords, query_records(coords=True), query.py --bin W --coords)
against the host restatement query_coords_ref.  Every comparison is exact equality of integer arrays, for bin_start,
bin_end and all binned arrays.  Coordinates do not depend on the tables: these are small random ones."""
import functools
import json
import os
import types

import numpy as np
import pytest

import gpu_support as gs
import oracle
import query_coords_inputs as qci
import query_bins_ref
import query_coords_ref
import query_ref
from gpu_support import Device, feed, index_cli, lib, run_py, same_coords

pytestmark = pytest.mark.gpu
CHUNK = qci.CHUNK


def _tables(k: int, n: int = 2, seed: int = 910):
    return gs.tables(k, n, seed)


@functools.lru_cache(maxsize=None)
def _want(name: str, k: int, W: int, fmt: str = "fasta"):
    """The reference of a text of query_coords_inputs, computed once and shared."""
    text = {"one": qci.one_record, "gapped": lambda: qci.gapped(k)[0], "blanks": qci.blanks, "many127": lambda: qci.many_records(127),
            "many200": lambda: qci.many_records(200), "short": qci.short_reads, "fastq": qci.fastq_reads}[name]()
    return text, query_coords_ref.expected(text, k, _tables(k), 1, 255, W, fmt)


def _coords(q, text: bytes, W: int, cuts=None):
    """One binned stream with coordinates through `q` (tables set); the indexer is reset behind it."""
    return gs.stream(q, text, bins=W, coords=True, cuts=cuts)


# ------------------------------------------------------------------ 1. one gap-free record ---------
@pytest.mark.parametrize("W", [1, 7, 128, 1000, 16384, 10 ** 9])
def test_one_gap_free_record(gpu, W):
    k = 9
    text, want = _want("one", k, W)
    query_coords_ref.check_consequences(want, k, W, gap_free=True)
    with Device(_tables(k)) as dev, lib().QueryIndexer(k, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        got = _coords(q, text, W)
    same_coords(got, want)
    b = np.arange(got["bin_start"].size, dtype=np.uint64)
    m = np.uint64(40_000 - k + 1)
    Wc = np.uint64(min(W, 1 << 40))
    assert np.array_equal(got["bin_start"], b * Wc) and np.array_equal(got["bin_end"], np.minimum((b + 1) * Wc, m) + np.uint64(k - 1))


# ------------------------------------------------------------------ 2. gaps ------------------------
@pytest.mark.parametrize("k", [5, 9])
def test_gaps(gpu, k):
    """Runs of N of length 1, k-1, k, 63, 64, 65 and 300 inside a piece, across piece and chunk seams, over a whole chunk,
    and at both ends of the record (query_coords_inputs.gapped)."""
    with Device(_tables(k)) as dev, lib().QueryIndexer(k, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        for W in (1, 5, 100, 5000):
            text, want = _want("gapped", k, W)
            query_coords_ref.check_consequences(want, k, W)
            assert int(want["bin_start"][0]) == 64 and int(want["bin_end"][-1]) == int(want["seq_len"][0]) - 65
            same_coords(_coords(q, text, W), want)


# ------------------------------------------------------------------ 3. blanks and line ends --------
@pytest.mark.parametrize("W", [1, 3, 50])
def test_blanks_and_line_ends(gpu, W):
    k = 5
    text, want = _want("blanks", k, W)
    assert len(want["records"]) == 6 and int(want["n_valid"][4]) == 0
    with Device(_tables(k)) as dev, lib().QueryIndexer(k, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        same_coords(_coords(q, text, W), want)
        same_coords(_coords(q, text, W, cuts=[5, 20 * qci.PIECE - 1, CHUNK - 2, CHUNK, 2 * CHUNK - 1, 3 * CHUNK - 1]), want)   # cuts inside the pending blanks


# ------------------------------------------------------------------ 4. many records ----------------
@pytest.mark.parametrize("s", [127, 200])
def test_many_records(gpu, s):
    """More than 64 records in a chunk, empty and shorter-than-k records between them, the long record behind them."""
    k = 5
    with Device(_tables(k)) as dev, lib().QueryIndexer(k, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        for W in (1, 3, 8, 1000):
            text, want = _want(f"many{s}", k, W)
            assert (want["n_valid"] == 0).sum() > 40
            query_coords_ref.check_consequences(want, k, W, gap_free=True)
            same_coords(_coords(q, text, W), want)


def test_short_reads_on_a_fresh_indexer_and_again_after_a_reset(gpu):
    """5 000 records in the first feed: the squeeze backs out, the arrays grow and the feed's kernels run again from the
    same position; the same text through the same indexer after a reset gives the same rows."""
    k, W = 5, 3
    text, want = _want("short", k, W)
    assert len(want["records"]) == 5000 > 4096
    with Device(_tables(k)) as dev, lib().QueryIndexer(k, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        first = _coords(q, text, W)
        same_coords(first, want)
        again = _coords(q, text, W)
        same_coords(again, want)
        halves = _coords(q, text, W, cuts=[len(text) // 2 + 1])
        same_coords(halves, want)


def test_short_reads_retry_in_the_second_feed(gpu):
    """The squeeze backs out in a later feed, while the accumulators and the coordinate rows hold the first feed's rows:
    the first feed ends inside record 100 after 9 bases (5 windows: one full row and an open row with a provisional end)
    and leaves the record array at its first capacity; the second brings the 5 000 records."""
    k, W = 5, 3
    text, want = _want("short", k, W)
    cut = 1612
    opened = text[:cut].count(b">")
    assert opened == 101 and text[cut - 12:cut - 9] == b">r\n"         # 9 bases of record 100: 9 - k + 1 = 5 windows
    assert int(query_coords_ref.expected(text[:cut], k, _tables(k), 1, 255, W)["n_valid"][100]) == 5
    assert opened + 2 * opened + 1024 < 4096                 # the first feed does not grow the record array ...
    assert len(want["records"]) == 5000 > 4096               # ... and the second does not fit in it
    with Device(_tables(k)) as dev, lib().QueryIndexer(k, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        same_coords(_coords(q, text, W, cuts=[cut]), want)


# ------------------------------------------------------------------ 5. feeds -----------------------
def _gap_cuts(k: int, W: int):
    text, runs = qci.gapped(k)
    _, want = _want("gapped", k, W)
    off = lambda b: qci.base_offset(qci.GAP_HEAD, b)         # noqa: E731
    lo, n = [r for r in runs if r[1] == 300][0]
    first_of_bin_2 = int(want["window_start"][2 * W])          # its last base is k - 1 further on
    cuts = sorted({2,                                        # inside the header
                   off(lo + 100),                            # inside a run of N
                   off(first_of_bin_2 + k - 1) + 1,          # directly after a bin's first window
                   len(text) - 2, len(text) - 1})            # one byte before the end of the record's last line, and of the record
    return text, want, cuts


@pytest.mark.parametrize("W", [5, 100, 5000])
def test_feeds(gpu, W):
    """The provisional end of the row that is open when a feed ends is overwritten by the feed that adds windows to it."""
    k = 9
    text, want, cuts = _gap_cuts(k, W)
    with Device(_tables(k)) as dev, lib().QueryIndexer(k, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        whole = _coords(q, text, W)
        same_coords(whole, want)
        for some in (cuts, cuts[1:2], cuts[2:3], [CHUNK, 2 * CHUNK + 1, 9 * CHUNK + 5000, 10 * CHUNK]):
            cut = _coords(q, text, W, cuts=some)
            for key in ("bin_start", "bin_end", "bin_hits", "bin_depth", "bin_first"):
                assert np.array_equal(cut[key], whole[key]), (key, some)


def test_more_than_1024_chunks_in_one_feed(gpu):
    """1025 chunks in one feed: k_coords_scan takes the chunks' pairs 1024 at a time, and the position at the first byte of
    chunk 1024 hangs on the first round's total.  One record without a gap runs across chunks 0 .. 1024;
    short records with a blank, an N and no window follow it in the last chunk.  The byte-wise yardstick would take
    a minute for 17 MB of text: it walks the text from the second header on (positions begin anew with every record), and
    the windows of the long record start at 0, 1, 2, ... -- what check_consequences(gap_free=True) states."""
    k = 5
    head = b">long\n"
    n_long = ((1024 * CHUNK + 3000 - len(head)) // (qci.WIDTH + 1)) * qci.WIDTH
    long_rec = query_ref._record(b"long", query_ref._bases(np.random.default_rng(905), n_long), qci.WIDTH)
    tail = b">t1\nACGTTGCAAC GTACGGTCAT\nACGNTTGACCA\n>t2\nACG\n>t3\n\n>t4\nTTGACGGTCATTGACCATG\n"
    text = long_rec + tail
    assert 1024 * CHUNK < len(long_rec) and -(-len(text) // CHUNK) == 1025      # the scan's second round: one chunk
    seq_len_t, n_win_t, starts_t = query_coords_ref.window_starts(tail, k)
    with Device(_tables(k)) as dev, lib().QueryIndexer(k, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        for W in (4099, 10 ** 9):
            want = query_bins_ref.expected(text, k, _tables(k), 1, 255, W)
            m = want["n_valid"]
            assert int(m[0]) == n_long - k + 1 and np.array_equal(m[1:], n_win_t) and np.array_equal(want["seq_len"][1:], seq_len_t)
            starts = np.concatenate([np.arange(int(m[0]), dtype=np.uint64), starts_t])
            want["bin_start"], want["bin_end"] = query_coords_ref.bin_coords(m, starts, k, W)
            query_coords_ref.check_consequences(want, k, W)
            assert int(want["bin_end"][want["row_record"] == 0][-1]) == n_long
            q.set_bins(W)
            q.set_coords(True)
            feed(q, text)
            assert q.timings()["feeds"] == 1, "the text was meant to be one feed of 1025 chunks"
            q.reset()
            same_coords(_coords(q, text, W), want)


# ------------------------------------------------------------------ 6. FASTQ -----------------------
def test_fastq_reads(gpu):
    k = 9
    with Device(_tables(k)) as dev, lib().QueryIndexer(k, device=0, fmt="fastq") as q:
        q.set_tables(dev.ptrs, 1, 255)
        for W in (2, 50):
            fq, want = _want("fastq", k, W, "fastq")
            assert len(want["records"]) == 300 and (want["n_valid"] == 0).any() and (want["n_valid"] > 50).any()
            query_coords_ref.check_consequences(want, k, W)
            same_coords(_coords(q, fq, W), want)
            same_coords(_coords(q, fq, W, cuts=[1, 10_003, CHUNK]), want)


# ------------------------------------------------------------------ 7. k = 17, more than 16 tables -
def test_k17_table_counted_on_the_gpu(gpu):
    k, W = 17, 1000
    lib = gs.lib()
    genomes = qci.k17_genomes()
    text = qci.k17_text()
    sparse = [query_ref.SparseTable(oracle.kmer_list(genomes[0], k))]
    want = query_coords_ref.expected(text, k, sparse, 1, 255, W)
    with lib.Indexer(k, device=0) as ix:
        ix.feed(genomes[0])
        ix.finish()
        with lib.QueryIndexer(k, device=0) as q:
            q.set_tables([ix.table_device_ptr()], 1, 255)
            got = _coords(q, text, W)
    same_coords(got, want)


def test_seventeen_tables_in_two_staging_groups(gpu, tmp_path):
    """17 tables through query_records: 16 are staged, then 1; the coordinates come from the first stream only and the
    hits columns are complete."""
    from pykmer_amd import query
    k, W = 5, 100
    text = qci.many_records(200)
    qf = tmp_path / "q.fa"
    qf.write_bytes(text)
    dense = _tables(k, 17, 911)
    tables = [types.SimpleNamespace(kmer_len=k, index_file=f"t{i}.kin", data_size=4 ** k, table=t) for i, t in enumerate(dense)]
    staged, with_coords = [], []

    def stage(group, device):
        dev = Device([g.table for g in group])
        staged.append(len(group))
        return query.Staged(dev.ptrs, dev.bufs)

    def run(*args, **kw):
        part = query.run_query(*args, **kw)
        with_coords.append("bin_start" in part)
        return part

    got = query.query_records(str(qf), tables, 2, 254, device=0, hbm_budget=16 * 4 ** k + 100, stage=stage, run=run, bin_windows=W, coords=True)
    assert staged == [16, 1] and with_coords == [True, False] and got["n_groups"] == 2 and got["coords_s"] > 0
    want = query_coords_ref.expected(text, k, dense, 2, 254, W)
    for key in ("bin_start", "bin_end", "bin_hits", "bin_depth", "bin_first", "hits", "depth", "n_valid", "seq_len"):
        assert got[key].dtype == np.uint64 and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key
    assert got["bin_hits"].shape[1] == 17


# ------------------------------------------------------------------ 8. CLI -------------------------
def test_cli_end_to_end(gpu, tmp_path):
    k, W = 9, 50
    kins, tables = index_cli(tmp_path, ("a", "b"), k)
    kins = [os.path.basename(kin) for kin in kins]
    text = qci.blanks() + qci.gapped(k)[0][:30_000] + b"\n"
    (tmp_path / "q.fa").write_bytes(text)
    want = query_coords_ref.expected(text, k, tables, 1, 255, W)
    run_py("query.py", "C", "q.fa", *kins, "--bin", str(W), "--coords", cwd=str(tmp_path))
    run_py("query.py", "P", "q.fa", *kins, "--bin", str(W), cwd=str(tmp_path))
    made = sorted(p.name for p in tmp_path.iterdir() if p.name.startswith(("C.", "P.")))
    assert made == [f"{p}.{e}" for p in "CP" for e in ("kmb", "kmb.json", "kmb.tsv", "kmq", "kmq.json", "kmq.tsv")]
    zc, zp = np.load(tmp_path / "C.kmb"), np.load(tmp_path / "P.kmb")
    # without --coords: the files of a binned run as they were
    assert sorted(zp.files) == ["bin_first", "bin_windows", "depth", "hits", "kmer_len", "max_count", "min_count", "n_valid", "seq_len"]
    meta_p = json.loads((tmp_path / "P.kmb.json").read_text())
    assert "coords" not in meta_p
    lines_p = (tmp_path / "P.kmb.tsv").read_text().split("\n")
    assert lines_p[0].split("\t")[:4] == ["record", "bin", "first_window", "n_windows"] and len(lines_p[0].split("\t")) == 6
    # with it: two more arrays, one more key, two more columns; everything else equal
    assert sorted(zc.files) == sorted(zp.files + ["bin_start", "bin_end"])
    for key in zp.files:
        assert np.array_equal(zc[key], zp[key]), key
    for key, src in (("bin_start", "bin_start"), ("bin_end", "bin_end"), ("hits", "bin_hits"), ("bin_first", "bin_first")):
        assert zc[key].dtype == np.uint64 and zc[key].shape == want[src].shape and np.array_equal(zc[key], want[src]), key
    meta_c = json.loads((tmp_path / "C.kmb.json").read_text())
    assert meta_c["coords"] is True and {**meta_c, "project_name": "P"} == {**meta_p, "coords": True}
    lines_c = (tmp_path / "C.kmb.tsv").read_text().split("\n")
    assert lines_c[0].split("\t") == lines_p[0].split("\t")[:4] + ["start", "end"] + lines_p[0].split("\t")[4:]
    assert len(lines_c) == len(lines_p) == int(want["bin_first"][-1]) + 2
    rows_c, rows_p = ([ln.split("\t") for ln in lines[1:-1]] for lines in (lines_c, lines_p))
    assert [r[:4] + r[6:] for r in rows_c] == rows_p
    assert np.array_equal(np.array([int(r[4]) for r in rows_c], dtype=np.uint64), zc["bin_start"])
    assert np.array_equal(np.array([int(r[5]) for r in rows_c], dtype=np.uint64), zc["bin_end"])
    assert (tmp_path / "C.kmq.tsv").read_bytes() == (tmp_path / "P.kmq.tsv").read_bytes()
    assert np.array_equal(np.load(tmp_path / "C.kmq")["hits"], np.load(tmp_path / "P.kmq")["hits"])
    r = run_py("query.py", "Z", "q.fa", *kins, "--coords", cwd=str(tmp_path), status=1)
    # (the device warms up on a thread of its own beside the argument checks: its chatter may follow the message)
    assert [ln for ln in r.stderr.splitlines() if ln.startswith("error: ") and "--bin" in ln]
    assert not [p for p in tmp_path.iterdir() if p.name.startswith("Z.")]


# ------------------------------------------------------------------ 9. state errors ----------------
def test_state_errors(gpu):
    lib = gs.lib()
    raw = lib.load()
    k, W = 5, 3
    text, want = _want("many127", k, W)
    one = np.zeros(1, dtype=np.uint64)
    with lib.Indexer(k, device=0) as ix:                     # not a query indexer
        assert raw.pk_query_set_coords(ix._h, 1) == lib.PK_ERR_STATE
    with Device(_tables(k)) as dev, lib.QueryIndexer(k, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        with pytest.raises(lib.PkError) as e:
            q.set_coords(True)                               # before the bins
        assert e.value.code == lib.PK_ERR_STATE
        q.set_bins(0)
        assert raw.pk_query_set_coords(q._h, 1) == lib.PK_ERR_STATE      # bins of 0 windows are no bins
        q.set_bins(W)
        q.set_coords(True)
        q.set_coords(False)                                  # any number of times before the first feed
        feed(q, text)
        with pytest.raises(lib.PkError) as e:
            q.set_coords(True)                               # after the first feed
        assert e.value.code == lib.PK_ERR_STATE
        fin = q.finish()
        with pytest.raises(lib.PkError) as e:
            q.bin_coords()                                   # coordinates are off
        assert e.value.code == lib.PK_ERR_STATE
        assert raw.pk_query_bin_coords(q._h, one.ctypes.data, one.ctypes.data, 1 << 40) == lib.PK_ERR_STATE
        hits, _, first = q.bin_results(fin["n_records"])     # the indexer is usable all the same
        assert np.array_equal(hits, want["bin_hits"]) and np.array_equal(first, want["bin_first"])
        # a reset clears the setting with the bins; set again, the same indexer delivers
        q.reset()
        q.set_bins(W)
        feed(q, text)
        q.finish()
        assert raw.pk_query_bin_coords(q._h, one.ctypes.data, one.ctypes.data, 1 << 40) == lib.PK_ERR_STATE
        q.reset()
        q.set_bins(W)
        q.set_coords(True)
        feed(q, text)
        with pytest.raises(lib.PkError) as e:
            q.bin_coords()                                   # before finish
        assert e.value.code == lib.PK_ERR_STATE
        q.finish()
        B = int(want["bin_first"][-1])
        start, end = np.zeros(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64)
        with pytest.raises(lib.PkError) as e:
            lib._check(raw.pk_query_bin_coords(q._h, start.ctypes.data, end.ctypes.data, B - 1))
        assert e.value.code == lib.PK_ERR_RECS_CAP and str(B) in str(e.value) and not start.any() and not end.any()
        lib._check(raw.pk_query_bin_coords(q._h, start.ctypes.data, end.ctypes.data, B))
        assert np.array_equal(start, want["bin_start"]) and np.array_equal(end, want["bin_end"])
