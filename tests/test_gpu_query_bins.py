"""GPU: binned query hits (pk_query_set_bins, query_records(bin_windows=), query.py --bin) against the host restatement
query_bins_ref.  Every comparison is exact equality of integer arrays.  Every case also runs the same indexer unbinned
after a reset: the per-record sums of the rows must equal it, and bin_first[R] must be the row count."""
import ctypes
import functools
import json
import os
import types

import numpy as np
import pytest

import oracle
import query_bins_ref
import gpu_support as gs
import query_ref
import synth
from gpu_support import Device, binned, feed, index_cli, lib, run_py, same_bins

pytestmark = pytest.mark.gpu
CHUNK = 16384
K = 9


# ------------------------------------------------------------------ 1. one record across slots -----
@functools.lru_cache(maxsize=None)
def _one_record() -> bytes:
    """One record of 40 000 bases on 60-column lines: three 16 KiB chunks."""
    text = query_ref._record(b"one record", query_ref._bases(np.random.default_rng(400), 40_000))
    assert 2 * CHUNK < len(text) < 3 * CHUNK
    return text


@pytest.mark.parametrize("W", [1, 7, 64, 127, 128, 129, 1000, 1024, 16384, 10 ** 9])
def test_one_record_across_slots(gpu, W):
    """W = 1 .. 127: more than 128 rows per slot (rows beyond the LDS accumulator go to HBM); 128 .. 1024: rows inside waves
    and across them; 16384: rows across slots; 10^9: one row for the record."""
    text, tables = _one_record(), gs.tables(K, 3, 401)
    with Device(tables) as dev, lib().QueryIndexer(K, device=0) as q:
        for mn, mx in ((1, 255), (2, 254)):
            q.set_tables(dev.ptrs, mn, mx)
            want = query_bins_ref.expected(text, K, tables, mn, mx, W)
            assert int(want["bin_first"][-1]) == -(-(40_000 - K + 1) // W)
            same_bins(binned(q, text, W), want)


# ------------------------------------------------------------------ 2. gaps ------------------------
@functools.lru_cache(maxsize=None)
def _gapped():
    """(text, start, first_base): the record of case 1 with runs of N of lengths 1, 8, 9 and 500, the last one lying across
    the first 16 KiB boundary of the text."""
    text = _one_record()
    head = text.index(b"\n") + 1
    seq = bytearray(text[head:].replace(b"\n", b""))
    at = (CHUNK - head) - (CHUNK - head) // 61               # the base at the boundary: 60 bases + '\n' per line
    for lo, n in ((1000, 1), (5000, 8), (9000, 9), (at - 230, 500)):
        seq[lo:lo + n] = b"N" * n
    gapped = query_ref._record(b"one record", bytes(seq))
    assert len(gapped) == len(text)
    start, straddles, first_base = query_ref.straddling_windows(gapped, K)
    assert at - 230 < first_base[CHUNK] < at + 270 and not (straddles == CHUNK).any() and (straddles == 2 * CHUNK).any()
    assert start.size == 40_000 - K + 1 - (1 + 8 + 9 + 500) - 4 * (K - 1)
    return gapped, start, first_base


def _first_window_of_slot(start, first_base, boundary: int) -> int:
    """The number of the first window that ends in the slot behind `boundary` (a window lies in the slot of its last base)."""
    return int(np.searchsorted(start, first_base[boundary] - K + 1))


def _gap_bin_sizes():
    _, start, first_base = _gapped()
    j1 = _first_window_of_slot(start, first_base, CHUNK)     # the first window behind the 500 N
    j2 = _first_window_of_slot(start, first_base, 2 * CHUNK)
    assert 15_000 < j1 < j2 - 15_000 and j2 + 1 < start.size
    # a bin begins exactly on the slot's first window (W = j), one window before it (W = j - 1: bin 1 begins at j - 1) and
    # one after; for the third slot also as the beginning of bin 2
    return [5, 97, 4099, j1 - 1, j1, j1 + 1, j2 - 1, j2, j2 + 1] + ([j2 // 2] if j2 % 2 == 0 else [(j2 - 1) // 2, (j2 + 1) // 2])


@pytest.mark.parametrize("W", _gap_bin_sizes())
def test_gaps(gpu, W):
    """Bins count valid windows: they continue across a run of N, and no window that holds an N is counted."""
    text, start, _ = _gapped()
    tables = gs.tables(K, 3, 401)
    want = query_bins_ref.expected(text, K, tables, 1, 255, W)
    assert int(want["n_valid"][0]) == start.size and int(want["bin_first"][-1]) == -(-start.size // W)
    with Device(tables) as dev, lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        same_bins(binned(q, text, W), want)


# ------------------------------------------------------------------ 3. many records ----------------
@pytest.mark.parametrize("s", [127, 129, 200])
def test_many_records(gpu, s):
    """Reads of 12 bases have four windows: W = 4 fills one bin exactly, 3 gives two bins, 5 and 1000 a partial one; records
    without a window get no row; the long record lies behind more than 128 short ones."""
    text, index = query_ref.long_after_short(s, seed=500 + s, ragged=True)
    tables = gs.tables(K, 2, 402)
    with Device(tables) as dev, lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 2, 255)
        for W in (1, 3, 4, 5, 1000):
            want = query_bins_ref.expected(text, K, tables, 2, 255, W)
            empty = want["n_valid"] == 0
            assert empty.sum() > 40 and np.array_equal(np.diff(want["bin_first"].astype(np.int64))[empty], np.zeros(empty.sum(), dtype=np.int64))
            assert int(want["bin_first"][index]) == (want["n_valid"][:index] > 0).sum() * (2 if W == 3 else 4 if W == 1 else 1) >= 84
            same_bins(binned(q, text, W), want)


# ------------------------------------------------------------------ 4. feeds -----------------------
def test_feeds_cut_anywhere_and_reset(gpu):
    text, _, _ = _gapped()
    tables = gs.tables(K, 3, 401)
    rng = np.random.default_rng(403)
    # a cut inside the header, a 1-byte piece, cuts at random offsets (all of them inside a bin of 97 windows or more)
    cuts = sorted({3, 4, 2 * CHUNK, *(int(c) for c in rng.integers(12, len(text) - 1, 6))})
    assert text.index(b"\n") > 4 and 4 - 3 == 1
    with Device(tables) as dev, lib().QueryIndexer(K, device=0) as q:
        q.set_tables(dev.ptrs, 1, 255)
        whole = binned(q, text, 97)
        same_bins(whole, query_bins_ref.expected(text, K, tables, 1, 255, 97))
        cut = binned(q, text, 97, cuts=cuts)
        for key in ("bin_hits", "bin_depth", "bin_first", "records"):
            assert np.array_equal(cut[key], whole[key]), key
        # another W after the reset, fed in other pieces
        same_bins(binned(q, text, 4099, cuts=[CHUNK + 1, len(text) - 1]), query_bins_ref.expected(text, K, tables, 1, 255, 4099))
        # and no bins after a reset: the per-record call answers as before, the binned one refuses
        feed(q, text, cuts)
        fin = q.finish()
        hits, depth = q.results(fin["n_records"])
        plain = query_ref.expected(text, K, tables, 1, 255)
        assert np.array_equal(hits, plain["hits"]) and np.array_equal(depth, plain["depth"])
        with pytest.raises(lib().PkError) as e:
            q.bin_results(fin["n_records"])
        assert e.value.code == lib().PK_ERR_STATE
        # with bins on, the per-record call refuses
        q.reset()
        q.set_bins(97)
        feed(q, text)
        fin = q.finish()
        with pytest.raises(lib().PkError) as e:
            q.results(fin["n_records"])
        assert e.value.code == lib().PK_ERR_STATE


# ------------------------------------------------------------------ 5. more than 16 tables ---------
def test_more_than_sixteen_tables_in_two_staging_groups(gpu, tmp_path):
    """20 tables through query_records: the budget stages 17 and then 3, so the first group also runs the lookup's own loop
    over groups of 16."""
    from pykmer_amd import query
    text, _ = query_ref.long_after_short(129, seed=629, ragged=True)
    qf = tmp_path / "q.fa"
    qf.write_bytes(text)
    dense = gs.tables(K, 20, 404)
    tables = [types.SimpleNamespace(kmer_len=K, index_file=f"t{i}.kin", data_size=4 ** K, table=t) for i, t in enumerate(dense)]
    staged = []

    def stage(group, device):
        dev = Device([g.table for g in group])
        staged.append(len(group))
        return query.Staged(dev.ptrs, dev.bufs)

    got = query.query_records(str(qf), tables, 2, 254, device=0, hbm_budget=17 * 4 ** K + 100, stage=stage, bin_windows=100)
    assert staged == [17, 3] and got["n_groups"] == 2 and got["bin_windows"] == 100
    want = query_bins_ref.expected(text, K, dense, 2, 254, 100)
    assert got["names"] == query_ref.names(text, want["records"])
    for key in ("bin_hits", "bin_depth", "bin_first", "hits", "depth", "n_valid", "seq_len"):
        assert got[key].dtype == np.uint64 and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key
    plain = query.query_records(str(qf), tables, 2, 254, device=0, hbm_budget=17 * 4 ** K + 100, stage=stage)
    assert np.array_equal(plain["hits"], got["hits"]) and np.array_equal(plain["depth"], got["depth"]) and "bin_first" not in plain
    assert int(got["bin_first"][-1]) == got["bin_hits"].shape[0]


# ------------------------------------------------------------------ 6. FASTQ -----------------------
def test_fastq_reads(gpu):
    rng = np.random.default_rng(405)
    out = []
    for i in range(400):
        n = int(rng.integers(1, 151))                        # reads below k bases are records without a window
        seq = np.frombuffer(b"ACGTACGTACGTN", dtype=np.uint8)[rng.integers(0, 13, n)].tobytes()
        nl = b"\r\n" if i % 3 == 0 else b"\n"                  # CRLF in part of the set
        out.append(b"@read%d extra" % i + nl + seq + nl + b"+" + nl + bytes(rng.integers(33, 74, n, dtype=np.uint8)) + nl)
    fq = b"".join(out)
    tables = gs.tables(K, 2, 406)
    with Device(tables) as dev, lib().QueryIndexer(K, device=0, fmt="fastq") as q:
        q.set_tables(dev.ptrs, 1, 255)
        for W in (2, 50):
            want = query_bins_ref.expected(fq, K, tables, 1, 255, W, fmt="fastq")
            assert len(want["records"]) == 400 and (want["n_valid"] == 0).any() and (want["n_valid"] > 50).any()
            same_bins(binned(q, fq, W), want)
            same_bins(binned(q, fq, W, cuts=[1, 20_003, CHUNK]), want)


# ------------------------------------------------------------------ 7. k = 13 and k = 17 -----------
def test_k13(gpu):
    k, W, text = 13, 1000, _one_record()
    tables = gs.tables(k, 1, 407)
    with Device(tables) as dev, lib().QueryIndexer(k, device=0) as q:
        q.set_tables(dev.ptrs, 1, 254)
        same_bins(binned(q, text, W), query_bins_ref.expected(text, k, tables, 1, 254, W))


def test_k17_table_counted_on_the_gpu(gpu):
    """The 64-bit instantiation of the lookup, against a table that was counted on the GPU and never left HBM."""
    k, W = 17, 1000
    lib = gs.lib()
    genomes = [synth.family(i, 200_000)[0] for i in range(2)]
    text = bytes(genomes[1]) + bytes(genomes[0])             # another family member, then the indexed genome itself
    sparse = [query_ref.SparseTable(oracle.kmer_list(genomes[0], k))]
    want = query_bins_ref.expected(text, k, sparse, 1, 255, W)
    with lib.Indexer(k, device=0) as ix:
        ix.feed(genomes[0])
        ix.finish()
        with lib.QueryIndexer(k, device=0) as q:
            q.set_tables([ix.table_device_ptr()], 1, 255)
            got = binned(q, text, W)
    same_bins(got, want)
    n_self = len(oracle.kmer_list(genomes[0], k, records=True)[1]["records"])
    self_rows = got["bin_hits"][int(got["bin_first"][-1 - n_self]):, 0]
    assert n_self >= 1 and np.array_equal(self_rows, want["row_windows"][-self_rows.size:].astype(np.uint64))   # every window of itself hits
    assert 0 < int(got["bin_hits"][:int(got["bin_first"][-1 - n_self]), 0].sum()) < int(want["n_valid"][:-n_self].sum())


# ------------------------------------------------------------------ 8. CLI -------------------------
def test_cli_end_to_end(gpu, tmp_path):
    k, W = 9, 500
    kins, tables = index_cli(tmp_path, ("a", "b"), k)
    kins = [os.path.basename(kin) for kin in kins]
    text = query_ref.long_after_short(50, seed=650, ragged=True)[0] + bytes(synth.family(1, 20_000)[0])
    (tmp_path / "q.fa").write_bytes(text)
    want = query_bins_ref.expected(text, k, tables, 2, 255, W)
    names = [n.strip() for n in query_ref.names(text, want["records"])]

    out = run_py("query.py", "P", "q.fa", *kins, "--bin", str(W), "--min-count", "2", cwd=str(tmp_path)).stdout
    assert f"{int(want['bin_first'][-1]):,d} bins" in out
    run_py("query.py", "plain", "q.fa", *kins, "--min-count", "2", cwd=str(tmp_path))
    made = sorted(p.name for p in tmp_path.iterdir() if p.name.startswith(("P.", "plain.")))
    assert made == ["P.kmb", "P.kmb.json", "P.kmb.tsv", "P.kmq", "P.kmq.json", "P.kmq.tsv", "plain.kmq", "plain.kmq.json", "plain.kmq.tsv"]
    # the .kmq trio is the one of a run without --bin
    zp, zq = np.load(tmp_path / "P.kmq"), np.load(tmp_path / "plain.kmq")
    assert sorted(zp.files) == sorted(zq.files)
    for key in zq.files:
        assert zp[key].dtype == zq[key].dtype and np.array_equal(zp[key], zq[key]), key
    for key in ("hits", "depth", "n_valid", "seq_len"):
        assert np.array_equal(zp[key], want[key]), key
    assert (tmp_path / "P.kmq.tsv").read_bytes() == (tmp_path / "plain.kmq.tsv").read_bytes()
    meta_q = json.loads((tmp_path / "P.kmq.json").read_text())
    assert {**meta_q, "project_name": "plain"} == json.loads((tmp_path / "plain.kmq.json").read_text())
    # the .kmb trio against the yardstick
    z = np.load(tmp_path / "P.kmb")
    assert sorted(z.files) == ["bin_first", "bin_windows", "depth", "hits", "kmer_len", "max_count", "min_count", "n_valid", "seq_len"]
    for key, src in (("hits", "bin_hits"), ("depth", "bin_depth"), ("bin_first", "bin_first"), ("n_valid", "n_valid"), ("seq_len", "seq_len")):
        assert z[key].dtype == np.uint64 and z[key].shape == want[src].shape and np.array_equal(z[key], want[src]), key
    assert (int(z["bin_windows"]), int(z["kmer_len"]), int(z["min_count"]), int(z["max_count"])) == (W, k, 2, 255)
    meta = json.loads((tmp_path / "P.kmb.json").read_text())
    assert sorted(meta) == sorted(list(meta_q) + ["bin_windows", "n_bins"])
    assert {key: meta[key] for key in meta_q} == meta_q and meta["bin_windows"] == W and meta["n_bins"] == int(want["bin_first"][-1])
    assert meta["records"] == names
    lines = (tmp_path / "P.kmb.tsv").read_text().split("\n")
    columns = (tmp_path / "P.kmq.tsv").read_text().split("\n")[0].split("\t")[3:]      # one per table, as in the .kmq.tsv
    assert len(columns) == 2 and lines[0].split("\t") == ["record", "bin", "first_window", "n_windows"] + columns
    assert lines[-1] == "" and len(lines) == meta["n_bins"] + 2
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert [r[0] for r in rows] == [names[i] for i in want["row_record"]]
    assert [[int(v) for v in r[1:4]] for r in rows] == [[int(b), int(b) * W, int(n)] for b, n in zip(want["row_bin"], want["row_windows"])]
    assert np.array_equal(np.array([[int(v) for v in r[4:]] for r in rows], dtype=np.uint64), want["bin_hits"])
    # nothing is overwritten, and a bin size below 1 is refused
    before = {p.name: p.read_bytes() for p in tmp_path.iterdir()}
    r = run_py("query.py", "P", "q.fa", *kins, "--bin", str(W), "--min-count", "2", cwd=str(tmp_path), status=1)
    assert r.stderr.splitlines()[-1].startswith("error: ") and "already exists" in r.stderr
    r = run_py("query.py", "Z", "q.fa", *kins, "--bin", "0", cwd=str(tmp_path), status=1)
    assert r.stderr.splitlines()[-1].startswith("error: ") and "bin size" in r.stderr
    assert {p.name: p.read_bytes() for p in tmp_path.iterdir()} == before


# ------------------------------------------------------------------ 9. state errors ----------------
def test_state_errors(gpu):
    lib = gs.lib()
    raw = lib.load()
    text, _ = query_ref.long_after_short(20, seed=720, ragged=True)
    tables = gs.tables(K, 2, 408)
    with lib.Indexer(K, device=0) as ix:                     # not a query indexer
        assert raw.pk_query_set_bins(ix._h, 5) == lib.PK_ERR_STATE
    with Device(tables) as dev, lib.QueryIndexer(K, device=0) as q:
        with pytest.raises(lib.PkError) as e:
            q.set_bins(5)                                    # before the tables
        assert e.value.code == lib.PK_ERR_STATE
        q.set_tables(dev.ptrs, 1, 255)
        q.set_bins(5)
        q.set_bins(0)
        q.set_bins(6)                                        # any number of times before the first feed
        q.feed(text)
        with pytest.raises(lib.PkError) as e:
            q.set_bins(5)                                    # after the first feed
        assert e.value.code == lib.PK_ERR_STATE
        with pytest.raises(lib.PkError) as e:
            q.bin_results(100)                               # before finish
        assert e.value.code == lib.PK_ERR_STATE
        one = np.zeros(1, dtype=np.uint64)
        assert raw.pk_query_bin_results(q._h, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 1) == lib.PK_ERR_STATE
        fin = q.finish()
        with pytest.raises(lib.PkError) as e:
            q.set_bins(5)                                    # after finish
        assert e.value.code == lib.PK_ERR_STATE
        want = query_bins_ref.expected(text, K, tables, 1, 255, 6)
        R, B = fin["n_records"], int(want["bin_first"][-1])
        assert R == len(want["records"]) and B > R > 5
        n_bins = ctypes.c_uint64(0)
        assert raw.pk_query_bin_count(q._h, ctypes.byref(n_bins)) == 0 and n_bins.value == B
        hits, depth = np.zeros((B, 2), dtype=np.uint64), np.zeros((B, 2), dtype=np.uint64)
        first = np.zeros(R + 1, dtype=np.uint64)
        for bins_cap, recs_cap in ((B - 1, R), (B, R - 1), (0, 0)):
            with pytest.raises(lib.PkError) as e:
                lib._check(raw.pk_query_bin_results(q._h, hits.ctypes.data, depth.ctypes.data, first.ctypes.data, bins_cap, recs_cap))
            assert e.value.code == lib.PK_ERR_RECS_CAP and str(B) in str(e.value) and str(R) in str(e.value)
            assert not hits.any() and not first.any()        # nothing was written
        lib._check(raw.pk_query_bin_results(q._h, hits.ctypes.data, depth.ctypes.data, first.ctypes.data, B, R))
        assert np.array_equal(hits, want["bin_hits"]) and np.array_equal(depth, want["bin_depth"]) and np.array_equal(first, want["bin_first"])
        got = q.bin_results(R)
        assert np.array_equal(got[0], hits) and np.array_equal(got[2], first)
        with pytest.raises(ValueError):
            q.set_bins(-1)
