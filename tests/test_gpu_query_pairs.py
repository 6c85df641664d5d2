"""GPU: the shared windows of every pair of tables per query row (pk_query_set_pairs, query_records(pairs=True), query.py
--pairs, pykmer_amd.qpairs) against the host restatement query_pairs_ref.  Every comparison is exact equality of integer
arrays.  Every run is also checked against itself: hits, depth (and bin_first) are what the same indexer gives for the same
text with the option off, and no pair shares more windows than either of its tables has."""
import functools
import json
import os

import numpy as np
import pytest

import gpu_support as gs
import oracle
import query_pairs_ref as ref
import query_ref
import synth
from fastq_qual_ref import mask_fastq_to_fasta
from gpu_support import Device, checked_pairs, feed, index_cli, lib, run_py

pytestmark = pytest.mark.gpu
CHUNK = 16384
K = 9
QPAIR_ROWS = 64                                              # kmer_query.hip: the rows of a slot whose pairs are tallied in LDS


# ------------------------------------------------------------------ 1. one record across three slots
@functools.lru_cache(maxsize=None)
def _long_text() -> bytes:
    rng = np.random.default_rng(900)
    return query_ref._record(b"one record", query_ref._bases(rng, 40_000))


@pytest.mark.parametrize("W", [None, 1, 7, 63, 64, 65, 1000, 1024, 16384, 10 ** 9])
def test_one_record_across_three_slots(gpu, W):
    """W = 1, 7: rows inside a thread, far more per slot than LDS holds; 63, 64, 65: rows around a thread's 16 windows and
    inside a wave; 1000, 1024: rows across waves; 16384: rows across slots; 10^9 and unbinned: one row for all three slots.
    N = 1 has no pair (an empty second axis), 16 fills every plane."""
    text = _long_text()
    assert 2 * CHUNK < len(text) < 3 * CHUNK
    tables = gs.tables(K, 16, 901)
    sums = {}
    with Device(tables) as dev, lib().QueryIndexer(K, device=0) as q:
        for N in (1, 2, 3, 16):
            for window in ((1, 255), (2, 5), (255, 255)):
                want = ref.expected(text, K, tables[:N], *window, W=W)
                assert want["shared"].shape[1] == N * (N - 1) // 2 and (N == 1 or want["shared"].any())
                q.set_tables(dev.ptrs[:N], *window)
                got = checked_pairs(q, text, want, W=W, bins_last=N == 3)
                sums[N, window] = got["shared"].sum(axis=0, dtype=np.uint64)
                if W is not None:                            # each record's rows sum to the unbinned run
                    per_record = gs.stream(q, text, pairs=True)
                    assert np.array_equal(ref.record_sums(got["shared"], got["bin_first"]), per_record["shared"])
    assert sums[16, (1, 255)].size == 120 and sums[16, (1, 255)].all()


# ------------------------------------------------------------------ 1b. the LDS-resident rows ------
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("s", [QPAIR_ROWS - 1, QPAIR_ROWS, QPAIR_ROWS + 1, 129, 200])
def test_long_record_behind_short_ones(gpu, s, ragged):
    """The 12 000-base record is row s of its slot (tests/test_query_host.py checks the layout): whole waves of it lie in
    one row, so their pairs are summed across the wave and added by one lane -- to the last row tallied in LDS, and to
    HBM directly for the first row beyond and for later ones; from 129 on the hits of the same wave go to HBM as well.
    N = 2, 3, 16: an even and an odd number of planes, and all sixteen (every plane register full).  W = 1000: the record has twelve rows."""
    text, index = query_ref.long_after_short(s, seed=980 + s, ragged=ragged, tail_len=4000)
    tables = gs.tables(K, 16, 901)
    with Device(tables) as dev, lib().QueryIndexer(K, device=0) as q:
        for N in (2, 3, 16):
            for window in ((1, 255), (255, 255)):
                q.set_tables(dev.ptrs[:N], *window)
                for W in (None, 1000):
                    want = ref.expected(text, K, tables[:N], *window, W=W)
                    rows = slice(index, index + 1) if W is None else slice(int(want["bin_first"][index]), int(want["bin_first"][index + 1]))
                    assert want["n_valid"][index] == 12_000 - K + 1 and want["shared"][rows].all()
                    assert W is None or rows.stop - rows.start == 12 and (ragged or rows.start == s)
                    checked_pairs(q, text, want, W=W)


# ------------------------------------------------------------------ 2. many rows per slot ----------
def _reads(n_reads: int, seed: int) -> bytes:
    """Reads of 0 .. 150 bases, among them reads shorter than k and reads that are all N."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTACGTACGTACGTN", dtype=np.uint8)
    out = []
    for i in range(n_reads):
        n = int(rng.integers(0, 151))
        seq = b"N" * n if i % 17 == 5 else alphabet[rng.integers(0, alphabet.size, n)].tobytes()
        out.append(b">r%d\n" % i + seq + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("W", [None, 16])
def test_many_reads_per_slot(gpu, W):
    text = _reads(5000, 910)
    tables = gs.tables(K, 5, 911)
    want = ref.expected(text, K, tables, 1, 254, W=W)
    assert len(want["records"]) == 5000 and (want["n_valid"] == 0).sum() > 400
    with Device(tables) as dev, lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 1, 254)
        got = checked_pairs(q, text, want, W=W)
    if W is None:
        assert not got["shared"][want["n_valid"] == 0].any()


def test_fastq_reads_masked_and_not(gpu):
    rng = np.random.default_rng(920)
    out = []
    for i in range(3000):
        n = int(rng.integers(1, 151))
        seq = np.frombuffer(b"ACGTACGTACGTN", dtype=np.uint8)[rng.integers(0, 13, n)].tobytes()
        nl = b"\r\n" if i % 3 == 0 else b"\n"
        out.append(b"@read%d extra" % i + nl + seq + nl + b"+" + nl + bytes(rng.integers(33, 74, n, dtype=np.uint8)) + nl)
    fq = b"".join(out)
    tables = gs.tables(K, 3, 921)
    with Device(tables) as dev:
        with lib().QueryIndexer(K, device=0, fmt="fastq") as q:
            q.set_tables(dev.ptrs, 1, 255)
            want = ref.expected(fq, K, tables, 1, 255, fmt="fastq")
            assert len(want["records"]) == 3000 and (want["n_valid"] == 0).any()
            checked_pairs(q, fq, want)
            checked_pairs(q, fq, ref.expected(fq, K, tables, 1, 255, W=16, fmt="fastq"), W=16, cuts=[20_003])
        T = 33 + 3
        fasta, masked = mask_fastq_to_fasta(fq, T)
        with lib().QueryIndexer(K, device=0, fmt="fastq", min_qual_byte=T) as q:
            q.set_tables(dev.ptrs, 1, 255)
            low = ref.expected(fasta, K, tables, 1, 255)
            assert masked > 1000 and 0 < int(low["n_valid"].sum()) < int(want["n_valid"].sum())
            checked_pairs(q, fq, low)
            checked_pairs(q, fq, ref.expected(fasta, K, tables, 1, 255, W=16), W=16)


# ------------------------------------------------------------------ 3. feeds, retries, state -------
def test_feeds_cut_inside_a_record_and_a_window(gpu):
    text = _long_text() + _reads(800, 930)
    tables = gs.tables(K, 4, 931)
    with Device(tables) as dev, lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 2, 254)
        for W in (None, 100):
            want = ref.expected(text, K, tables, 2, 254, W=W)
            uncut = checked_pairs(q, text, want, W=W)
            cut = checked_pairs(q, text, want, W=W, cuts=[7, 8, 5000, 5003, CHUNK, CHUNK + 5, 2 * CHUNK - 3, len(text) - 40, len(text) - 1])
            assert np.array_equal(cut["shared"], uncut["shared"])


def test_retried_feeds_count_nothing_twice(gpu):
    """A fresh indexer whose first feed opens more records than the record array holds: the squeeze backs out, the arrays
    grow and the feed runs again; the second feed does the same."""
    lib = gs.lib()
    text = query_ref.reads_text(K, n_reads=24_000, seed=941)
    at = text.index(b">r5000\n")
    assert text[:at].count(b">") == 5000 > 4096
    tables = gs.tables(K, 3, 942)
    for W in (None, 5):
        want = ref.expected(text, K, tables, 1, 255, W=W)
        with Device(tables) as dev, lib.QueryIndexer(K, device=0) as q:
            q.set_tables(dev.ptrs, 1, 255)
            if W is not None:
                q.set_bins(W)
            q.set_pairs(True)
            feed(q, text, [at])                             # 5000 records, then 19 000 more: both feeds outgrow the array
            fin = q.finish()
            assert fin["n_records"] == 24_000
            rows = fin["n_records"] if W is None else int(q.bin_results(fin["n_records"])[2][-1])
            assert np.array_equal(q.pairs(rows), want["shared"])


def test_state_errors_and_reset(gpu):
    lib = gs.lib()
    raw = lib.load()
    text, _ = query_ref.long_after_short(20, seed=950, ragged=True)
    tables = gs.tables(K, 3, 951)
    one = np.zeros(1, dtype=np.uint64)
    with lib.Indexer(K, device=0) as ix:                     # not a query indexer
        assert raw.pk_query_set_pairs(ix._h, 1) == lib.PK_ERR_STATE
        assert raw.pk_query_pairs(ix._h, one.ctypes.data, 1) == lib.PK_ERR_STATE
    with Device(tables) as dev, lib.QueryIndexer(K, device=0) as q:
        with pytest.raises(lib.PkError) as e:
            q.set_pairs(True)                                # before the tables
        assert e.value.code == lib.PK_ERR_STATE and "pk_query_set_tables" in str(e.value)
        q.set_tables(dev.ptrs * 6, 1, 255)                   # 18 tables
        assert raw.pk_query_set_pairs(q._h, 1) == lib.PK_ERR_ARG
        with pytest.raises(ValueError, match="at most 16 tables"):
            q.set_pairs(True)
        q.set_tables(dev.ptrs, 1, 255)
        q.set_pairs(True)
        q.set_pairs(False)
        q.set_pairs(True)                                    # any number of times before the first feed
        with pytest.raises(ValueError, match="separate streams"):
            q.set_spectrum(True)                             # the two do not go together
        q.feed(text)
        with pytest.raises(lib.PkError) as e:
            q.set_pairs(True)                                # after the first feed
        assert e.value.code == lib.PK_ERR_STATE and "before the first feed" in str(e.value)
        with pytest.raises(lib.PkError) as e:
            q.pairs(100)                                     # before finish
        assert e.value.code == lib.PK_ERR_STATE
        fin = q.finish()
        want = ref.expected(text, K, tables, 1, 255)
        R = fin["n_records"]
        out = np.zeros((R, 3), dtype=np.uint64)
        for cap in (R - 1, 0):
            with pytest.raises(lib.PkError) as e:
                lib._check(raw.pk_query_pairs(q._h, out.ctypes.data, cap))
            assert e.value.code == lib.PK_ERR_RECS_CAP and str(R) in str(e.value) and not out.any()
        lib._check(raw.pk_query_pairs(q._h, out.ctypes.data, R))
        assert np.array_equal(out, want["shared"]) and np.array_equal(q.pairs(R), out)
        q.reset()
        q.feed(text)                                         # the setting went with the reset
        q.finish()
        assert raw.pk_query_pairs(q._h, out.ctypes.data, R) == lib.PK_ERR_STATE
        with pytest.raises(lib.PkError) as e:
            q.pairs(R)
        assert e.value.code == lib.PK_ERR_STATE and "pk_query_set_pairs" in str(e.value)
        q.reset()
        q.set_pairs(True)                                    # a second stream on the same indexer: nothing carried over
        q.feed(text)
        q.finish()
        assert np.array_equal(q.pairs(R), want["shared"])


def test_two_equal_tables_share_their_hits(gpu):
    text = _long_text() + _reads(500, 960)
    a, b = gs.tables(K, 2, 961)
    tables = (a, b, a.copy())
    with Device(tables) as dev, lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 2, 254)
        for W in (None, 50):
            got = checked_pairs(q, text, ref.expected(text, K, tables, 2, 254, W=W), W=W)
            assert np.array_equal(got["shared"][:, 1], got["hits"][:, 0]) and got["hits"][:, 0].any()       # pair (0, 2)
            assert np.array_equal(got["shared"][:, 0], got["shared"][:, 2])                                 # (0, 1) and (1, 2)


# ------------------------------------------------------------------ 4. k = 15, k = 17 --------------
@pytest.mark.parametrize("k", [15, 17])
def test_tables_counted_on_the_gpu(gpu, k):
    """The 32-bit (k = 15) and the 64-bit (k = 17) instantiation, against tables that were counted on the GPU and never left
    HBM; the reference reads them as SparseTables."""
    lib = gs.lib()
    genomes = [bytes(synth.family(i, 60_000)[0]) for i in range(2)]
    text = genomes[1] + genomes[0]
    sparse = [query_ref.SparseTable(oracle.kmer_list(g, k)) for g in genomes]
    with lib.Indexer(k, device=0) as a, lib.Indexer(k, device=0) as b:
        for ix, g in zip((a, b), genomes):
            ix.feed(g)
            ix.finish()
        with lib.QueryIndexer(k, device=0) as q:
            q.set_tables([ix.table_device_ptr() for ix in (a, b)], 1, 255)
            got = checked_pairs(q, text, ref.expected(text, k, sparse, 1, 255))
            checked_pairs(q, text, ref.expected(text, k, sparse, 1, 255, W=1000), W=1000)
    assert got["shared"].any()


# ------------------------------------------------------------------ 5. CLI -------------------------
def _run(*argv, cwd, status=0):
    return run_py(*argv, cwd=cwd, status=status, env=gs.env_with_root())


def test_cli_end_to_end(gpu, tmp_path):
    kins, tables = index_cli(tmp_path, ("a", "b", "c"), K)
    kins = [os.path.basename(kin) for kin in kins]
    text = query_ref.long_after_short(30, seed=970, ragged=True)[0] + bytes(synth.family(1, 20_000)[0])
    (tmp_path / "q.fa").write_bytes(text)
    before = {p.name for p in tmp_path.iterdir()}
    r = _run("query.py", "P", "q.fa", *kins, "--pairs", cwd=str(tmp_path))
    assert r.stdout.strip().splitlines()[-1].endswith(", 3 pairs")
    _run("query.py", "B", "q.fa", *kins, "--bin", "50", "--coords", "--pairs", cwd=str(tmp_path))
    _run("query.py", "D", "q.fa", *kins, "--bin", "50", "--coords", cwd=str(tmp_path))        # without the option: the files as before
    trio, kmb = ["kmq", "kmq.json", "kmq.tsv"], ["kmb", "kmb.json", "kmb.tsv"]
    kmp = ["kmp", "kmp.json", "kmp.tsv"]
    made = sorted(p.name for p in tmp_path.iterdir() if p.name not in before)
    assert made == sorted([f"P.{e}" for e in trio + kmp] + [f"B.{e}" for e in trio + kmb + kmp] + [f"D.{e}" for e in trio + kmb])
    for ext in trio + kmb:                                   # .kmq and .kmb are written exactly as without the option
        if ext.endswith(".json"):
            assert {**json.loads((tmp_path / f"B.{ext}").read_text()), "project_name": "D"} == json.loads((tmp_path / f"D.{ext}").read_text()), ext
        elif ext.endswith(".tsv"):
            assert (tmp_path / f"B.{ext}").read_bytes() == (tmp_path / f"D.{ext}").read_bytes(), ext
        else:
            zb, zd = np.load(tmp_path / f"B.{ext}"), np.load(tmp_path / f"D.{ext}")
            assert sorted(zb.files) == sorted(zd.files), ext
            for key in zd.files:
                assert zb[key].dtype == zd[key].dtype and np.array_equal(zb[key], zd[key]), (ext, key)
    for proj, W in (("P", None), ("B", 50)):
        want = ref.expected(text, K, tables, 1, 255, W=W)
        z = np.load(tmp_path / f"{proj}.kmp")
        more = [] if W is None else ["bin_first", "bin_windows", "bin_start", "bin_end"]
        assert sorted(z.files) == sorted(["shared", "hits", "pairs", "n_valid", "seq_len", "kmer_len", "min_count", "max_count"] + more)
        assert z["shared"].dtype == np.uint64 and np.array_equal(z["shared"], want["shared"]) and want["shared"].any()
        assert z["hits"].dtype == np.uint64 and np.array_equal(z["hits"], want["hits"])
        assert z["pairs"].dtype == np.int32 and z["pairs"].tolist() == [[0, 1], [0, 2], [1, 2]]
        assert np.array_equal(z["n_valid"], want["n_valid"]) and (int(z["kmer_len"]), int(z["min_count"]), int(z["max_count"])) == (K, 1, 255)
        meta = json.loads((tmp_path / f"{proj}.kmp.json").read_text())
        src = json.loads((tmp_path / (f"{proj}.kmq.json" if W is None else f"{proj}.kmb.json")).read_text())
        assert {key: meta[key] for key in meta if key != "n_pairs"} == src and meta["n_pairs"] == 3
        lines = (tmp_path / f"{proj}.kmp.tsv").read_text().split("\n")
        lead_src = (tmp_path / (f"{proj}.kmq.tsv" if W is None else f"{proj}.kmb.tsv")).read_text().split("\n")
        lead = 3 if W is None else 6
        cols = lead_src[0].split("\t")[lead:]                # the tables' names, as the .kmq / .kmb head their columns
        assert len(cols) == 3 and lines[0].split("\t")[:lead] == lead_src[0].split("\t")[:lead]
        assert lines[0].split("\t")[lead:] == [f"{cols[i]}|{cols[j]}" for i, j in ((0, 1), (0, 2), (1, 2))]
        assert len(lines) == len(lead_src) == want["shared"].shape[0] + 2 and lines[-1] == ""
        assert [ln.split("\t")[:lead] for ln in lines[1:-1]] == [ln.split("\t")[:lead] for ln in lead_src[1:-1]]
        assert np.array_equal(np.array([[int(v) for v in ln.split("\t")[lead:]] for ln in lines[1:-1]], dtype=np.uint64).reshape(-1, 3), want["shared"])
    # one row as a .kma: the genome record of the query, by index and by name, and a bin of it
    from pykmer_amd import distance, qpairs
    want = ref.expected(text, K, tables, 1, 255)
    row = len(want["records"]) - 1
    _run("-m", "pykmer_amd.qpairs", "P.kmp", "R", "--row", str(row), cwd=str(tmp_path))
    m = np.load(tmp_path / "R.001-255.kma")["matrix"]
    assert np.array_equal(m, qpairs.row_matrix(want["hits"][row], want["shared"][row])) and m[0, 1, 2] == want["shared"][row, 0]
    assert distance.load(tmp_path / "R.001-255.kma").shape[0] == 3
    name = json.loads((tmp_path / "B.kmp.json").read_text())["records"][row]
    _run("-m", "pykmer_amd.qpairs", "B.kmp", "S", "--record", name, "--bin", "2", cwd=str(tmp_path))
    binned = ref.expected(text, K, tables, 1, 255, W=50)
    at = int(binned["bin_first"][row]) + 2
    assert np.array_equal(np.load(tmp_path / "S.001-255.kma")["matrix"], qpairs.row_matrix(binned["hits"][at], binned["shared"][at]))
    # refusals: nothing written
    listing = sorted(p.name for p in tmp_path.iterdir())
    r = _run("query.py", "X", "q.fa", *kins, "--pairs", "--spectrum", cwd=str(tmp_path), status=1)
    assert [ln for ln in r.stderr.splitlines() if ln.startswith("error: ")]
    (tmp_path / "only.kmp.tsv").write_bytes(b"")
    r = _run("query.py", "only", "q.fa", *kins, "--pairs", cwd=str(tmp_path), status=1)
    assert [ln for ln in r.stderr.splitlines() if ln.startswith("error: ") and "already exists" in ln]
    (tmp_path / "only.kmp.tsv").unlink()
    assert sorted(p.name for p in tmp_path.iterdir()) == listing
