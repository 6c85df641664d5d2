"""GPU: per-record and per-bin count spectra of the query lookup (pk_query_set_spectrum, query_records(spectrum=True),
query.py --spectrum, pykmer_amd.qspectrum) against the host restatement query_spectrum_ref.  Every comparison is exact
equality of integer arrays.  Every run is also checked against itself: each row's spectrum sums to the row's windows, the
run's own count window taken from the spectrum gives the run's hits and depth, and hits, depth (and bin_first) are what
the same indexer gives for the same text with the option off."""
import functools
import json
import types

import numpy as np
import pytest

import gpu_support as gs
import inputs
import oracle
import query_ref
import query_spectrum_ref as ref
import synth
from fastq_qual_ref import mask_fastq_to_fasta
from gpu_support import Device, checked_spectrum, feed, index_cli, lib, run_py

pytestmark = pytest.mark.gpu
CHUNK = 16384
K = 9
QSPEC_ROWS = 32                                              # kmer_query.hip (test_query_spectrum_host.py checks the mirror)


# ------------------------------------------------------------------ 1. edge grammar ----------------
@pytest.mark.parametrize("k", [1, 5, 9])
def test_edge_grammar(gpu, k):
    tables = gs.tables(k, 3, 800 + k)
    with Device(tables) as dev, lib().QueryIndexer(k, device=0) as q:
        for i, text in enumerate((inputs.edge_fasta(), inputs.byte_soup(40_000, 11), inputs.byte_soup(40_000, 12))):
            want = ref.expected(text, k, tables)
            for window in ((1, 255), (2, 254)) if i == 0 else ((2, 254),):
                q.set_tables(dev.ptrs, *window)
                checked_spectrum(q, text, window, want)
            if i == 0:
                assert (want["n_valid"] == 0).any() and not want["spectrum"][want["n_valid"] == 0].any()
                assert want["spectrum"][..., 0].any() and want["spectrum"][..., 255].any()


# ------------------------------------------------------------------ 2. one record across slots -----
@pytest.mark.parametrize("k", [9, 13])
def test_slot_seams(gpu, k):
    """One record of 100 000 bases over seven slots, an N next to two chunk seams: every wave lies in one row (the counts
    are summed across the wave) and seven slots add to the same 256 counters per table."""
    text = query_ref.seam_text(k)
    assert len(text) > 6 * CHUNK
    if k == 9:
        tables = gs.tables(k, 2, 821)
    else:                                                    # 64 MiB each: cheap to fill, the window's edges frequent
        pool = np.array([0, 1, 254, 255, 7, 0, 1, 255], dtype=np.uint8)
        tables = [np.tile(np.roll(pool, i), 4 ** k // 8) for i in range(2)]
        tables[1] = np.roll(tables[1], 3)
    want = ref.expected(text, k, tables)
    assert want["spectrum"].shape == (1, 2, 256)
    with Device(tables) as dev, lib().QueryIndexer(k, device=0) as q:
        q.set_tables(dev.ptrs, 2, 254)
        checked_spectrum(q, text, (2, 254), want)
        checked_spectrum(q, text, (2, 254), want, cuts=[2 * CHUNK - 3, 5 * CHUNK + 3])


# ------------------------------------------------------------------ 3. the LDS-resident rows --------
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("s", [QSPEC_ROWS - 1, QSPEC_ROWS, QSPEC_ROWS + 1, 200])
def test_long_record_behind_short_ones(gpu, s, ragged):
    """The 12 000-base record is row s of its slot: the last row tallied in LDS, the first and a later one tallied in HBM;
    ragged: records without a window are rows all the same."""
    text, index = query_ref.long_after_short(s, seed=830 + s, ragged=ragged)
    tables = gs.tables(K, 2, 822)
    want = ref.expected(text, K, tables)
    assert want["n_valid"][index] == 12_000 - K + 1 and (not ragged or (want["n_valid"] == 0).sum() >= s // 3)
    with Device(tables) as dev, lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        checked_spectrum(q, text, (1, 255), want)


# ------------------------------------------------------------------ 4. many rows per thread --------
def test_many_records_per_piece_and_chunk(gpu):
    """Reads of 0, 1, k-1, k, k+1, 40 ... bases: several rows inside one thread's 16 windows; 6000 records are beyond the
    record array's first capacity, so the spectra grow with it."""
    text = query_ref.reads_text(K)
    tables = gs.tables(K, 2, 832)
    want = ref.expected(text, K, tables)
    assert len(want["records"]) == 6000 and (want["n_valid"] == 0).sum() > 1000
    with Device(tables) as dev, lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 1, 254)
        got = checked_spectrum(q, text, (1, 254), want)
    assert not got["spectrum"][want["n_valid"] == 0].any()


# ------------------------------------------------------------------ 5. one count dominates ---------
def test_tables_in_which_one_count_dominates(gpu):
    """All zero, all 255 and a random table: every window of the first two meets in one counter per row."""
    rng = np.random.default_rng(850)
    text = query_ref._record(b"long", query_ref._bases(rng, 40_000)) + b"".join(b">a\n" + query_ref._bases(rng, 12) + b"\n" for _ in range(300))
    tables = (np.zeros(4 ** K, dtype=np.uint8), np.full(4 ** K, 255, dtype=np.uint8), gs.tables(K, 1, 851)[0])
    want = ref.expected(text, K, tables)
    m = want["n_valid"]
    assert m.size == 301 and m[0] == 40_000 - K + 1 and (m[1:] == 12 - K + 1).all()
    assert np.array_equal(want["spectrum"][:, 0, 0], m) and np.array_equal(want["spectrum"][:, 1, 255], m)
    with Device(tables) as dev, lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        got = checked_spectrum(q, text, (1, 255), want)
        for W in (100, 3):
            checked_spectrum(q, text, (1, 255), ref.expected(text, K, tables, W), W=W)
    assert int(got["spectrum"].sum()) == 3 * int(m.sum())


# ------------------------------------------------------------------ 6. feeds -----------------------
def test_feeds_cut_anywhere_and_reset(gpu):
    lib = gs.lib()
    reads, seams = query_ref.reads_text(K), query_ref.seam_text(K)
    tables = gs.tables(K, 2, 841)
    want_reads, want_seams = ref.expected(reads, K, tables), ref.expected(seams, K, tables)
    at = reads.index(b">r5000\n")
    assert reads[:at].count(b">") == 5000 > 4096             # the first feed alone outgrows the record array: it runs twice
    r = reads[:5000].count(b">")
    assert 3 * r + 1024 <= 4096                              # cut at byte 5000 the array grows in the second feed, over live rows
    with Device(tables) as dev:
        with lib.QueryIndexer(K, device=0) as q:             # a fresh indexer
            q.set_tables(dev.ptrs, 2, 255)
            checked_spectrum(q, reads, (2, 255), want_reads, cuts=[at])
            checked_spectrum(q, reads, (2, 255), want_reads, cuts=[5000])
            hdr = reads.find(b">", 3 * CHUNK + 100) + 2      # inside a header
            checked_spectrum(q, reads, (2, 255), want_reads, cuts=sorted({7, 8, CHUNK, CHUNK + 5, 2 * CHUNK - 3, 3 * CHUNK, hdr, len(reads) - 1}))
            checked_spectrum(q, seams, (2, 255), want_seams, cuts=[7, 8, CHUNK, CHUNK + 5, 2 * CHUNK - 3, 4 * CHUNK + 61 * 3 + 4, len(seams) - 1])
        with lib.QueryIndexer(K, device=0) as q:
            q.set_tables(dev.ptrs, 2, 255)
            q.set_spectrum(True)
            feed(q, reads, [at])
            fin = q.finish()
            first = q.spectrum(fin["n_records"]).copy()
            q.reset()                                        # a second stream on the same indexer: nothing carried over
            q.set_spectrum(True)
            feed(q, seams, [CHUNK + 1])
            fin = q.finish()
            second = q.spectrum(fin["n_records"]).copy()
            q.reset()                                        # and the setting is off again
            feed(q, seams)
            fin = q.finish()
            hits, _ = q.results(fin["n_records"])
            with pytest.raises(lib.PkError) as e:
                q.spectrum(fin["n_records"])
            assert e.value.code == lib.PK_ERR_STATE
        assert np.array_equal(first, want_reads["spectrum"]) and np.array_equal(second, want_seams["spectrum"])
        assert np.array_equal(hits, ref.window(want_seams["spectrum"], 2, 255)[0])


def test_binned_feeds_grow_the_records_and_the_rows_over_live_spectra(gpu):
    """Bins of 4 windows with the spectra on, in two feeds: cut at byte 5000 the record array grows inside the second feed,
    cut at record 5000 inside both, and every time the rows of hits, depth and the spectra move with live contents."""
    reads, tables = query_ref.reads_text(K), gs.tables(K, 3, 843)
    want = ref.expected(reads, K, tables, 4)
    at = reads.index(b">r5000\n")
    assert 3 * reads[:5000].count(b">") + 1024 <= 4096 < reads[:at].count(b">") == 5000
    assert int(want["bin_first"][-1]) > 5000 // 4 + 4096 + 1                 # more rows than the first feed was sized for
    with Device(tables) as dev, lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 2, 255)
        for cut in (5000, at):
            checked_spectrum(q, reads, (2, 255), want, W=4, cuts=[cut], bins_last=cut == at)


# ------------------------------------------------------------------ 7. one table, seventeen --------
def test_one_table_and_seventeen(gpu):
    """N = 17: the lookup runs once for 16 tables and once for the last; column t is the run against table t alone."""
    text, _ = query_ref.long_after_short(40, seed=870, ragged=True)
    tables = gs.tables(K, 17, 871)
    want = ref.expected(text, K, tables)
    with Device(tables) as dev, lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 2, 254)
        got = checked_spectrum(q, text, (2, 254), want)
        binned = checked_spectrum(q, text, (2, 254), ref.expected(text, K, tables, 100), W=100)
        assert got["spectrum"].shape[1:] == binned["spectrum"].shape[1:] == (17, 256)
        for t in range(17):
            q.set_tables(dev.ptrs[t:t + 1], 2, 254)
            one = gs.stream(q, text, spectrum=True)
            assert one["spectrum"].shape == (len(want["records"]), 1, 256)
            assert np.array_equal(one["spectrum"][:, 0], got["spectrum"][:, t]), t
            assert np.array_equal(one["hits"][:, 0], got["hits"][:, t]), t


# ------------------------------------------------------------------ 8. bins ------------------------
@functools.lru_cache(maxsize=None)
def _bins_text(long_record: bool) -> bytes:
    """Short reads and two records of 12 000 and 3 000 bases; long_record: and one of 40 000 bases over three slots."""
    rng = np.random.default_rng(880)
    text = query_ref.long_after_short(40, seed=881, ragged=True)[0]
    return text + query_ref._record(b"one record", query_ref._bases(rng, 40_000)) if long_record else text


@pytest.mark.parametrize("W", [1, 7, 100, 20_000])
def test_bins(gpu, W):
    """W = 1, 7: far more rows per slot than LDS holds; 100: rows inside waves; 20 000: a row across slots.  Each record's
    rows sum to its per-record spectrum, and bin_first is what it is without the option (_checked)."""
    text, tables = _bins_text(W >= 100), gs.tables(K, 3, 882)
    want = ref.expected(text, K, tables, W)
    per_record = ref.expected(text, K, tables)
    assert np.array_equal(ref.record_sums(want["spectrum"], want["bin_first"]), per_record["spectrum"])      # (the yardsticks agree)
    assert int(want["bin_first"][-1]) > len(want["records"]) - (want["n_valid"] == 0).sum()
    with Device(tables) as dev, lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 2, 254)
        got = checked_spectrum(q, text, (2, 254), want, W=W, bins_last=W in (7, 20_000))
        rec = gs.stream(q, text, spectrum=True)
    assert np.array_equal(ref.record_sums(got["spectrum"], got["bin_first"]), rec["spectrum"])
    assert np.array_equal(rec["spectrum"], per_record["spectrum"])


# ------------------------------------------------------------------ 9. k = 17 ----------------------
def test_k17_table_counted_on_the_gpu(gpu):
    """The 64-bit instantiation, against a table that was counted on the GPU and never left HBM."""
    k = 17
    lib = gs.lib()
    genomes = [synth.family(i, 200_000)[0] for i in range(2)]
    text = bytes(genomes[1]) + bytes(genomes[0])             # another family member, then the indexed genome itself
    sparse = [query_ref.SparseTable(oracle.kmer_list(genomes[0], k))]
    with lib.Indexer(k, device=0) as ix:
        ix.feed(genomes[0])
        ix.finish()
        with lib.QueryIndexer(k, device=0) as q:
            q.set_tables([ix.table_device_ptr()], 1, 255)
            got = checked_spectrum(q, text, (1, 255), ref.expected(text, k, sparse))
            checked_spectrum(q, text, (1, 255), ref.expected(text, k, sparse, 1000), W=1000)
    assert got["spectrum"][-1, 0, 0] == 0 and got["spectrum"][0, 0, 0] > 0      # every window of the genome itself is in its table


# ------------------------------------------------------------------ 10. FASTQ ----------------------
def test_fastq_reads(gpu):
    rng = np.random.default_rng(890)
    out = []
    for i in range(400):
        n = int(rng.integers(1, 151))                        # reads below k bases are records without a window
        seq = np.frombuffer(b"ACGTACGTACGTN", dtype=np.uint8)[rng.integers(0, 13, n)].tobytes()
        nl = b"\r\n" if i % 3 == 0 else b"\n"
        out.append(b"@read%d extra" % i + nl + seq + nl + b"+" + nl + bytes(rng.integers(33, 74, n, dtype=np.uint8)) + nl)
    fq = b"".join(out)
    tables = gs.tables(K, 2, 891)
    with Device(tables) as dev:
        with lib().QueryIndexer(K, device=0, fmt="fastq") as q:
            q.set_tables(dev.ptrs, 1, 255)
            want = ref.expected(fq, K, tables, fmt="fastq")
            assert len(want["records"]) == 400 and (want["n_valid"] == 0).any()
            checked_spectrum(q, fq, (1, 255), want)
            checked_spectrum(q, fq, (1, 255), want, cuts=[1, 20_003, CHUNK])
            checked_spectrum(q, fq, (1, 255), ref.expected(fq, K, tables, 50, fmt="fastq"), W=50)
        T = 33 + 3
        fasta, masked = mask_fastq_to_fasta(fq, T)
        with lib().QueryIndexer(K, device=0, fmt="fastq", min_qual_byte=T) as q:
            q.set_tables(dev.ptrs, 1, 255)
            low = ref.expected(fasta, K, tables)
            assert masked > 1000 and 0 < int(low["n_valid"].sum()) < int(want["n_valid"].sum())
            checked_spectrum(q, fq, (1, 255), low, cuts=[20_003])


# ------------------------------------------------------------------ 11. CLI ------------------------
@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    """Two k = 9 tables indexed by the CLI, once for both CLI cases: (directory, kin names, host tables, query text)."""
    base = tmp_path_factory.mktemp("qspec_cli")
    kins, tables = index_cli(base, ("a", "b"), K)
    text = query_ref.long_after_short(50, seed=650, ragged=True)[0] + bytes(synth.family(1, 20_000)[0])
    (base / "q.fa").write_bytes(text)
    return base, kins, tables, text


@pytest.mark.parametrize("W", [None, 500])
def test_cli_end_to_end(gpu, cli_inputs, tmp_path, W):
    base, kins, tables, text = cli_inputs
    qfa = str(base / "q.fa")
    bins = [] if W is None else ["--bin", str(W)]
    want = ref.expected(text, K, tables, W)
    names = [n.strip() for n in query_ref.names(text, want["records"])]
    run_py("query.py", "P", qfa, *kins, "--spectrum", *bins, cwd=str(tmp_path))
    run_py("query.py", "D", qfa, *kins, "--min-count", "2", "--max-count", "200", *bins, cwd=str(tmp_path))     # no --spectrum: the files as before
    trio = ["kmq", "kmq.json", "kmq.tsv"] + ([] if W is None else ["kmb", "kmb.json", "kmb.tsv"])
    made = sorted(p.name for p in tmp_path.iterdir())
    assert made == sorted([f"D.{e}" for e in trio] + [f"P.{e}" for e in trio + ["kmh", "kmh.json", "kmh.tsv"]])
    # the .kmh trio against the yardstick
    z = np.load(tmp_path / "P.kmh")
    assert sorted(z.files) == sorted(["spectrum", "median", "n_valid", "seq_len", "kmer_len"] + ([] if W is None else ["bin_first", "bin_windows"]))
    assert z["spectrum"].dtype == np.uint64 and np.array_equal(z["spectrum"], want["spectrum"])
    assert z["median"].dtype == np.uint8 and np.array_equal(z["median"], want["median"]) and want["median"].any()
    assert np.array_equal(z["n_valid"], want["n_valid"]) and np.array_equal(z["seq_len"], want["seq_len"]) and int(z["kmer_len"]) == K
    if W is not None:
        assert np.array_equal(z["bin_first"], want["bin_first"]) and z["bin_first"].dtype == np.uint64 and int(z["bin_windows"]) == W
    meta, meta_q = json.loads((tmp_path / "P.kmh.json").read_text()), json.loads((tmp_path / "P.kmq.json").read_text())
    more = {} if W is None else {"bin_windows": W, "n_bins": int(want["bin_first"][-1])}
    assert sorted(meta) == sorted([key for key in meta_q if key not in ("min_count", "max_count")] + list(more))
    assert {key: meta[key] for key in meta if key not in more} == {key: meta_q[key] for key in meta if key not in more}
    assert {key: meta[key] for key in more} == more and meta["records"] == names
    lead = 3 if W is None else 4
    src = (tmp_path / ("P.kmq.tsv" if W is None else "P.kmb.tsv")).read_text().split("\n")
    lines = (tmp_path / "P.kmh.tsv").read_text().split("\n")
    assert len(lines) == len(src) == want["spectrum"].shape[0] + 2 and lines[0] == src[0] and lines[-1] == ""
    assert [ln.split("\t")[:lead] for ln in lines[1:-1]] == [ln.split("\t")[:lead] for ln in src[1:-1]]
    assert np.array_equal(np.array([[int(v) for v in ln.split("\t")[lead:]] for ln in lines[1:-1]], dtype=np.uint8).reshape(-1, 2), want["median"])
    # qspectrum at the second window, without tables or a GPU, writes what the direct run wrote
    run_py("-m", "pykmer_amd.qspectrum", "P.kmh", "S", "--min-count", "2", "--max-count", "200", cwd=str(tmp_path), env=gs.env_with_root())
    for ext in trio:
        if ext.endswith(".json"):
            assert {**json.loads((tmp_path / f"S.{ext}").read_text()), "project_name": "D"} == json.loads((tmp_path / f"D.{ext}").read_text()), ext
        elif ext.endswith(".tsv"):
            assert (tmp_path / f"S.{ext}").read_bytes() == (tmp_path / f"D.{ext}").read_bytes(), ext
        else:
            zs, zd = np.load(tmp_path / f"S.{ext}"), np.load(tmp_path / f"D.{ext}")
            assert sorted(zs.files) == sorted(zd.files), ext
            for key in zd.files:
                assert zs[key].dtype == zd[key].dtype and np.array_equal(zs[key], zd[key]), (ext, key)
    # nothing is overwritten
    before = {p.name: p.read_bytes() for p in tmp_path.iterdir()}
    (tmp_path / "only.kmh.tsv").write_bytes(b"")
    r = run_py("query.py", "only", qfa, *kins, "--spectrum", *bins, cwd=str(tmp_path), status=1)
    assert [ln for ln in r.stderr.splitlines() if ln.startswith("error: ") and "already exists" in ln]     # (the device may warm up and speak beside it)
    (tmp_path / "only.kmh.tsv").unlink()
    assert {p.name: p.read_bytes() for p in tmp_path.iterdir()} == before


def test_query_records_concatenates_table_groups(gpu, tmp_path):
    """20 tables staged as 17 and 3: spectrum, median and their binned forms concatenate along the table axis."""
    from pykmer_amd import query
    text, _ = query_ref.long_after_short(40, seed=899, ragged=True)
    qf = tmp_path / "q.fa"
    qf.write_bytes(text)
    dense = gs.tables(K, 20, 898)
    tables = [types.SimpleNamespace(kmer_len=K, index_file=f"t{i}.kin", data_size=4 ** K, table=t) for i, t in enumerate(dense)]

    def stage(group, device):
        dev = Device([g.table for g in group])
        return query.Staged(dev.ptrs, dev.bufs)

    got = query.query_records(str(qf), tables, 2, 254, device=0, hbm_budget=17 * 4 ** K + 100, stage=stage, bin_windows=100, spectrum=True)
    want, per_record = ref.expected(text, K, dense, 100), ref.expected(text, K, dense)
    assert got["n_groups"] == 2
    for key, src in (("bin_spectrum", want["spectrum"]), ("spectrum", per_record["spectrum"]), ("bin_median", want["median"]),
                     ("median", per_record["median"])):
        assert got[key].dtype == src.dtype and got[key].shape == src.shape and np.array_equal(got[key], src), key
    ref.check_identities(got["bin_spectrum"], want["row_windows"], got["bin_hits"], got["bin_depth"], 2, 254)
    ref.check_identities(got["spectrum"], per_record["row_windows"], got["hits"], got["depth"], 2, 254)


# ------------------------------------------------------------------ 12. state errors ---------------
def test_state_errors(gpu):
    lib = gs.lib()
    raw = lib.load()
    text, _ = query_ref.long_after_short(20, seed=720, ragged=True)
    tables = gs.tables(K, 2, 808)
    one = np.zeros(1, dtype=np.uint64)
    with lib.Indexer(K, device=0) as ix:                     # not a query indexer
        assert raw.pk_query_set_spectrum(ix._h, 1) == lib.PK_ERR_STATE
        assert raw.pk_query_spectrum(ix._h, one.ctypes.data, 1) == lib.PK_ERR_STATE
    with Device(tables) as dev, lib.QueryIndexer(K, device=0) as q:
        with pytest.raises(lib.PkError) as e:
            q.set_spectrum(True)                             # before the tables
        assert e.value.code == lib.PK_ERR_STATE and "pk_query_set_tables" in str(e.value)
        q.set_tables(dev.ptrs, 1, 255)
        q.set_spectrum(True)
        q.set_spectrum(False)
        q.set_spectrum(True)                                 # any number of times before the first feed
        q.feed(text)
        with pytest.raises(lib.PkError) as e:
            q.set_spectrum(True)                             # after the first feed
        assert e.value.code == lib.PK_ERR_STATE and "before the first feed" in str(e.value)
        with pytest.raises(lib.PkError) as e:
            q.spectrum(100)                                  # before finish
        assert e.value.code == lib.PK_ERR_STATE
        fin = q.finish()
        with pytest.raises(lib.PkError) as e:
            q.set_spectrum(True)                             # after finish
        assert e.value.code == lib.PK_ERR_STATE
        want = ref.expected(text, K, tables)
        R = fin["n_records"]
        out = np.zeros((R, 2, 256), dtype=np.uint64)
        for cap in (R - 1, 0):
            with pytest.raises(lib.PkError) as e:
                lib._check(raw.pk_query_spectrum(q._h, out.ctypes.data, cap))
            assert e.value.code == lib.PK_ERR_RECS_CAP and str(R) in str(e.value) and not out.any()
        lib._check(raw.pk_query_spectrum(q._h, out.ctypes.data, R))
        assert np.array_equal(out, want["spectrum"]) and np.array_equal(q.spectrum(R), out)
        q.reset()
        q.feed(text)                                         # the setting went with the reset
        q.finish()
        assert raw.pk_query_spectrum(q._h, out.ctypes.data, R) == lib.PK_ERR_STATE
        q.reset()
        q.set_spectrum(True)
        q.set_spectrum(False)                                # switched off before the first feed: off
        q.feed(text)
        q.finish()
        with pytest.raises(lib.PkError) as e:
            q.spectrum(R)
        assert e.value.code == lib.PK_ERR_STATE and "pk_query_set_spectrum" in str(e.value)
