"""GPU: per-record and per-bin count spectra of the query lookup (pk_query_set_spectrum, query_records(spectrum=True),
query.py --spectrum, pykmer_amd.qspectrum) against the host restatement query_spectrum_ref.  Every comparison is exact
equality of integer arrays.  Every run is also checked against itself: each row's spectrum sums to the row's windows, the
run's own count window taken from the spectrum gives the run's hits and depth, and hits, depth (and bin_first) are what
the same indexer gives for the same text with the option off."""
import functools
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import inputs
import oracle
import query_ref
import query_spectrum_ref as ref
import synth
from fastq_qual_ref import mask_fastq_to_fasta
from test_gpu_query import _reads_text, _seam_text

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 16384
K = 9
QSPEC_ROWS = 32                                              # kmer_query.hip (test_query_spectrum_host.py checks the mirror)


def _lib():
    from pykmer_amd import _lib as lib
    return lib


class _Device:
    """Host tables staged in HBM for the length of a test."""

    def __init__(self, tables):
        self.bufs = [_lib().DeviceBuffer(t.size, 0) for t in tables]
        for b, t in zip(self.bufs, tables):
            b.upload(t)
        self.ptrs = [b.ptr for b in self.bufs]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()


def _feed(q, text: bytes, cuts=None):
    buf = np.frombuffer(text, dtype=np.uint8)
    pos = 0
    for c in list(cuts or []) + [len(text)]:
        if c > pos:
            q.feed(buf[pos:c])
            pos = c


def _stream(q, text: bytes, W=None, spectrum=True, cuts=None, bins_last=False):
    """One stream through `q` (tables set), then a reset.  bins_last: pk_query_set_spectrum before pk_query_set_bins."""
    if W is not None and not bins_last:
        q.set_bins(W)
    if spectrum:
        q.set_spectrum(True)
    if W is not None and bins_last:
        q.set_bins(W)
    _feed(q, text, cuts)
    fin = q.finish()
    n = fin["n_records"]
    out = {"fin": fin, "n_valid": q.records(n)["n_valid_kmers"].astype(np.uint64)}
    if W is None:
        hits, depth = q.results(n)
        rows = n
    else:
        hits, depth, first = q.bin_results(n)
        rows = int(first[-1])
        out["bin_first"] = first.copy()
    out.update(hits=hits.copy(), depth=depth.copy())
    if spectrum:
        out["spectrum"] = q.spectrum(rows).copy()
    q.reset()
    return out


def _checked(q, text: bytes, window, want: dict, W=None, cuts=None, bins_last=False):
    """A stream with the option on and one with it off through `q` (tables set with `window`); the identities, the
    unchanged tallies, and the spectrum against the yardstick."""
    got = _stream(q, text, W, True, cuts, bins_last)
    plain = _stream(q, text, W, False)
    for key in ("hits", "depth", "n_valid") + (("bin_first",) if W is not None else ()):
        assert np.array_equal(got[key], plain[key]), key
    assert np.array_equal(got["n_valid"], want["n_valid"]) and got["fin"]["num_kmers"] == int(want["n_valid"].sum())
    if W is not None:
        assert np.array_equal(got["bin_first"], want["bin_first"])
    ref.check_identities(got["spectrum"], want["row_windows"], got["hits"], got["depth"], *window)
    assert got["spectrum"].shape == want["spectrum"].shape
    assert np.array_equal(got["spectrum"], want["spectrum"]), np.argwhere(got["spectrum"] != want["spectrum"])[:5]
    return got


@functools.lru_cache(maxsize=None)
def _tables(k: int, n: int, seed: int):
    return tuple(query_ref.random_tables(k, n, seed))


# ------------------------------------------------------------------ 1. edge grammar ----------------
@pytest.mark.parametrize("k", [1, 5, 9])
def test_edge_grammar(gpu, k):
    tables = _tables(k, 3, 800 + k)
    with _Device(tables) as dev, _lib().QueryIndexer(k, device=0) as q:
        for i, text in enumerate((inputs.edge_fasta(), inputs.byte_soup(40_000, 11), inputs.byte_soup(40_000, 12))):
            want = ref.expected(text, k, tables)
            for window in ((1, 255), (2, 254)) if i == 0 else ((2, 254),):
                q.set_tables(dev.ptrs, *window)
                _checked(q, text, window, want)
            if i == 0:
                assert (want["n_valid"] == 0).any() and not want["spectrum"][want["n_valid"] == 0].any()
                assert want["spectrum"][..., 0].any() and want["spectrum"][..., 255].any()


# ------------------------------------------------------------------ 2. one record across slots -----
@pytest.mark.parametrize("k", [9, 13])
def test_slot_seams(gpu, k):
    """One record of 100 000 bases over seven slots, an N next to two chunk seams: every wave lies in one row (the counts
    are summed across the wave) and seven slots add to the same 256 counters per table."""
    text = _seam_text(k)
    assert len(text) > 6 * CHUNK
    if k == 9:
        tables = _tables(k, 2, 821)
    else:                                                    # 64 MiB each: cheap to fill, the window's edges frequent
        pool = np.array([0, 1, 254, 255, 7, 0, 1, 255], dtype=np.uint8)
        tables = [np.tile(np.roll(pool, i), 4 ** k // 8) for i in range(2)]
        tables[1] = np.roll(tables[1], 3)
    want = ref.expected(text, k, tables)
    assert want["spectrum"].shape == (1, 2, 256)
    with _Device(tables) as dev, _lib().QueryIndexer(k, device=0) as q:
        q.set_tables(dev.ptrs, 2, 254)
        _checked(q, text, (2, 254), want)
        _checked(q, text, (2, 254), want, cuts=[2 * CHUNK - 3, 5 * CHUNK + 3])


# ------------------------------------------------------------------ 3. the LDS-resident rows --------
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("s", [QSPEC_ROWS - 1, QSPEC_ROWS, QSPEC_ROWS + 1, 200])
def test_long_record_behind_short_ones(gpu, s, ragged):
    """The 12 000-base record is row s of its slot: the last row tallied in LDS, the first and a later one tallied in HBM;
    ragged: records without a window are rows all the same."""
    text, index = query_ref.long_after_short(s, seed=830 + s, ragged=ragged)
    tables = _tables(K, 2, 822)
    want = ref.expected(text, K, tables)
    assert want["n_valid"][index] == 12_000 - K + 1 and (not ragged or (want["n_valid"] == 0).sum() >= s // 3)
    with _Device(tables) as dev, _lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        _checked(q, text, (1, 255), want)


# ------------------------------------------------------------------ 4. many rows per thread --------
def test_many_records_per_piece_and_chunk(gpu):
    """Reads of 0, 1, k-1, k, k+1, 40 ... bases: several rows inside one thread's 16 windows; 6000 records are beyond the
    record array's first capacity, so the spectra grow with it."""
    text = _reads_text(K)
    tables = _tables(K, 2, 832)
    want = ref.expected(text, K, tables)
    assert len(want["records"]) == 6000 and (want["n_valid"] == 0).sum() > 1000
    with _Device(tables) as dev, _lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 1, 254)
        got = _checked(q, text, (1, 254), want)
    assert not got["spectrum"][want["n_valid"] == 0].any()


# ------------------------------------------------------------------ 5. one count dominates ---------
def test_tables_in_which_one_count_dominates(gpu):
    """All zero, all 255 and a random table: every window of the first two meets in one counter per row."""
    rng = np.random.default_rng(850)
    text = query_ref._record(b"long", query_ref._bases(rng, 40_000)) + b"".join(b">a\n" + query_ref._bases(rng, 12) + b"\n" for _ in range(300))
    tables = (np.zeros(4 ** K, dtype=np.uint8), np.full(4 ** K, 255, dtype=np.uint8), _tables(K, 1, 851)[0])
    want = ref.expected(text, K, tables)
    m = want["n_valid"]
    assert m.size == 301 and m[0] == 40_000 - K + 1 and (m[1:] == 12 - K + 1).all()
    assert np.array_equal(want["spectrum"][:, 0, 0], m) and np.array_equal(want["spectrum"][:, 1, 255], m)
    with _Device(tables) as dev, _lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        got = _checked(q, text, (1, 255), want)
        for W in (100, 3):
            _checked(q, text, (1, 255), ref.expected(text, K, tables, W), W=W)
    assert int(got["spectrum"].sum()) == 3 * int(m.sum())


# ------------------------------------------------------------------ 6. feeds -----------------------
def test_feeds_cut_anywhere_and_reset(gpu):
    lib = _lib()
    reads, seams = _reads_text(K), _seam_text(K)
    tables = _tables(K, 2, 841)
    want_reads, want_seams = ref.expected(reads, K, tables), ref.expected(seams, K, tables)
    at = reads.index(b">r5000\n")
    assert reads[:at].count(b">") == 5000 > 4096             # the first feed alone outgrows the record array: it runs twice
    r = reads[:5000].count(b">")
    assert 3 * r + 1024 <= 4096                              # cut at byte 5000 the array grows in the second feed, over live rows
    with _Device(tables) as dev:
        with lib.QueryIndexer(K, device=0) as q:             # a fresh indexer
            q.set_tables(dev.ptrs, 2, 255)
            _checked(q, reads, (2, 255), want_reads, cuts=[at])
            _checked(q, reads, (2, 255), want_reads, cuts=[5000])
            hdr = reads.find(b">", 3 * CHUNK + 100) + 2      # inside a header
            _checked(q, reads, (2, 255), want_reads, cuts=sorted({7, 8, CHUNK, CHUNK + 5, 2 * CHUNK - 3, 3 * CHUNK, hdr, len(reads) - 1}))
            _checked(q, seams, (2, 255), want_seams, cuts=[7, 8, CHUNK, CHUNK + 5, 2 * CHUNK - 3, 4 * CHUNK + 61 * 3 + 4, len(seams) - 1])
        with lib.QueryIndexer(K, device=0) as q:
            q.set_tables(dev.ptrs, 2, 255)
            q.set_spectrum(True)
            _feed(q, reads, [at])
            fin = q.finish()
            first = q.spectrum(fin["n_records"]).copy()
            q.reset()                                        # a second stream on the same indexer: nothing carried over
            q.set_spectrum(True)
            _feed(q, seams, [CHUNK + 1])
            fin = q.finish()
            second = q.spectrum(fin["n_records"]).copy()
            q.reset()                                        # and the setting is off again
            _feed(q, seams)
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
    reads, tables = _reads_text(K), _tables(K, 3, 843)
    want = ref.expected(reads, K, tables, 4)
    at = reads.index(b">r5000\n")
    assert 3 * reads[:5000].count(b">") + 1024 <= 4096 < reads[:at].count(b">") == 5000
    assert int(want["bin_first"][-1]) > 5000 // 4 + 4096 + 1                 # more rows than the first feed was sized for
    with _Device(tables) as dev, _lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 2, 255)
        for cut in (5000, at):
            _checked(q, reads, (2, 255), want, W=4, cuts=[cut], bins_last=cut == at)


# ------------------------------------------------------------------ 7. one table, seventeen --------
def test_one_table_and_seventeen(gpu):
    """N = 17: the lookup runs once for 16 tables and once for the last; column t is the run against table t alone."""
    text, _ = query_ref.long_after_short(40, seed=870, ragged=True)
    tables = _tables(K, 17, 871)
    want = ref.expected(text, K, tables)
    with _Device(tables) as dev, _lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 2, 254)
        got = _checked(q, text, (2, 254), want)
        binned = _checked(q, text, (2, 254), ref.expected(text, K, tables, 100), W=100)
        assert got["spectrum"].shape[1:] == binned["spectrum"].shape[1:] == (17, 256)
        for t in range(17):
            q.set_tables(dev.ptrs[t:t + 1], 2, 254)
            one = _stream(q, text)
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
    text, tables = _bins_text(W >= 100), _tables(K, 3, 882)
    want = ref.expected(text, K, tables, W)
    per_record = ref.expected(text, K, tables)
    assert np.array_equal(ref.record_sums(want["spectrum"], want["bin_first"]), per_record["spectrum"])      # (the yardsticks agree)
    assert int(want["bin_first"][-1]) > len(want["records"]) - (want["n_valid"] == 0).sum()
    with _Device(tables) as dev, _lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 2, 254)
        got = _checked(q, text, (2, 254), want, W=W, bins_last=W in (7, 20_000))
        rec = _stream(q, text)
    assert np.array_equal(ref.record_sums(got["spectrum"], got["bin_first"]), rec["spectrum"])
    assert np.array_equal(rec["spectrum"], per_record["spectrum"])


# ------------------------------------------------------------------ 9. k = 17 ----------------------
def test_k17_table_counted_on_the_gpu(gpu):
    """The 64-bit instantiation, against a table that was counted on the GPU and never left HBM."""
    k = 17
    lib = _lib()
    genomes = [synth.family(i, 200_000)[0] for i in range(2)]
    text = bytes(genomes[1]) + bytes(genomes[0])             # another family member, then the indexed genome itself
    sparse = [query_ref.SparseTable(oracle.kmer_list(genomes[0], k))]
    with lib.Indexer(k, device=0) as ix:
        ix.feed(genomes[0])
        ix.finish()
        with lib.QueryIndexer(k, device=0) as q:
            q.set_tables([ix.table_device_ptr()], 1, 255)
            got = _checked(q, text, (1, 255), ref.expected(text, k, sparse))
            _checked(q, text, (1, 255), ref.expected(text, k, sparse, 1000), W=1000)
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
    tables = _tables(K, 2, 891)
    with _Device(tables) as dev:
        with _lib().QueryIndexer(K, device=0, fmt="fastq") as q:
            q.set_tables(dev.ptrs, 1, 255)
            want = ref.expected(fq, K, tables, fmt="fastq")
            assert len(want["records"]) == 400 and (want["n_valid"] == 0).any()
            _checked(q, fq, (1, 255), want)
            _checked(q, fq, (1, 255), want, cuts=[1, 20_003, CHUNK])
            _checked(q, fq, (1, 255), ref.expected(fq, K, tables, 50, fmt="fastq"), W=50)
        T = 33 + 3
        fasta, masked = mask_fastq_to_fasta(fq, T)
        with _lib().QueryIndexer(K, device=0, fmt="fastq", min_qual_byte=T) as q:
            q.set_tables(dev.ptrs, 1, 255)
            low = ref.expected(fasta, K, tables)
            assert masked > 1000 and 0 < int(low["n_valid"].sum()) < int(want["n_valid"].sum())
            _checked(q, fq, (1, 255), low, cuts=[20_003])


# ------------------------------------------------------------------ 11. CLI ------------------------
def _run(*argv, cwd, status=0):
    r = subprocess.run([sys.executable] + list(argv), cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == status, r.stdout[-2000:] + r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    """Two k = 9 tables indexed by the CLI, once for both CLI cases: (directory, kin names, host tables, query text)."""
    base = tmp_path_factory.mktemp("qspec_cli")
    kins, tables = [], []
    for name in ("a", "b"):
        data = bytes(synth.family(len(kins), 20_000)[0])
        (base / f"{name}.fa").write_bytes(data)
        _run(os.path.join(ROOT, "indexer.py"), f"{name}.fa", name, str(K), cwd=str(base))
        kins.append(os.path.join(str(base), f"{name}.fa.{K:02d}.kin"))
        tables.append(oracle.count_fasta(data, K)["table"])
    text = query_ref.long_after_short(50, seed=650, ragged=True)[0] + bytes(synth.family(1, 20_000)[0])
    (base / "q.fa").write_bytes(text)
    return base, kins, tables, text


@pytest.mark.parametrize("W", [None, 500])
def test_cli_end_to_end(gpu, cli_inputs, tmp_path, W):
    base, kins, tables, text = cli_inputs
    qfa, query_py = str(base / "q.fa"), os.path.join(ROOT, "query.py")
    bins = [] if W is None else ["--bin", str(W)]
    want = ref.expected(text, K, tables, W)
    names = [n.strip() for n in query_ref.names(text, want["records"])]
    _run(query_py, "P", qfa, *kins, "--spectrum", *bins, cwd=str(tmp_path))
    _run(query_py, "D", qfa, *kins, "--min-count", "2", "--max-count", "200", *bins, cwd=str(tmp_path))     # no --spectrum: the files as before
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
    r = subprocess.run([sys.executable, "-m", "pykmer_amd.qspectrum", "P.kmh", "S", "--min-count", "2", "--max-count", "200"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
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
    r = _run(query_py, "only", qfa, *kins, "--spectrum", *bins, cwd=str(tmp_path), status=1)
    assert [ln for ln in r.stderr.splitlines() if ln.startswith("error: ") and "already exists" in ln]     # (the device may warm up and speak beside it)
    (tmp_path / "only.kmh.tsv").unlink()
    assert {p.name: p.read_bytes() for p in tmp_path.iterdir()} == before


def test_query_records_concatenates_table_groups(gpu, tmp_path):
    """20 tables staged as 17 and 3: spectrum, median and their binned forms concatenate along the table axis."""
    from pykmer_amd import query
    text, _ = query_ref.long_after_short(40, seed=899, ragged=True)
    qf = tmp_path / "q.fa"
    qf.write_bytes(text)
    dense = _tables(K, 20, 898)
    tables = [types.SimpleNamespace(kmer_len=K, index_file=f"t{i}.kin", data_size=4 ** K, table=t) for i, t in enumerate(dense)]

    def stage(group, device):
        dev = _Device([g.table for g in group])
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
    lib = _lib()
    raw = lib.load()
    text, _ = query_ref.long_after_short(20, seed=720, ragged=True)
    tables = _tables(K, 2, 808)
    one = np.zeros(1, dtype=np.uint64)
    with lib.Indexer(K, device=0) as ix:                     # not a query indexer
        assert raw.pk_query_set_spectrum(ix._h, 1) == lib.PK_ERR_STATE
        assert raw.pk_query_spectrum(ix._h, one.ctypes.data, 1) == lib.PK_ERR_STATE
    with _Device(tables) as dev, lib.QueryIndexer(K, device=0) as q:
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
