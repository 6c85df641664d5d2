"""CPU: the query's shared windows per pair of tables -- the yardstick (query_pairs_ref), pykmer_amd.qpairs, query_records and
the CLI with a substituted stage / run, the `.kmp` writer and the refusals.  No call here touches a GPU."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import inputs
import oracle
import query_bins_ref
import query_pairs_ref as ref
import query_ref
from gpu_support import env_with_root, run_py
from host_support import query_hooks
from pykmer_amd import _lib, distance, qpairs, query, spectrum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the yardstick ------------------
def test_pairs_ref_against_a_brute_force_loop():
    k, mn, mx = 3, 2, 254
    text = b">a\nACGTTGCAAGGTNACGTACGT\n>empty\n\n>b\nAC\n>c\nGGGTTTACGTAAAACCC\nACGT\n"
    tables = query_ref.random_tables(k, 4, seed=5)
    kmers, info = oracle.kmer_list(text, k, records=True)
    n_valid = [int(v) for v in info["records"]["n_valid_kmers"]]
    assert n_valid.count(0) == 2 and len(n_valid) == 4
    for W in (None, 1, 4, 100):
        want = ref.expected(text, k, tables, mn, mx, W=W)
        rows, at = [], 0                                     # the rows as lists of k-mers, window by window
        for m in n_valid:
            rec = [int(a) for a in kmers[at:at + m]]
            at += m
            if W is None:
                rows.append(rec)
            else:
                rows += [rec[b:b + W] for b in range(0, m, W)]
        assert want["shared"].shape == (len(rows), 6) and want["pairs"].tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
        assert np.array_equal(want["pairs"], spectrum.pair_list(4))
        for r, row in enumerate(rows):
            for t in range(4):
                assert int(want["hits"][r, t]) == sum(1 for a in row if mn <= tables[t][a] <= mx)
            for p, (i, j) in enumerate(want["pairs"]):
                assert int(want["shared"][r, p]) == sum(1 for a in row if mn <= tables[i][a] <= mx and mn <= tables[j][a] <= mx), (W, r, p)
        ref.check_identities(want["shared"], want["hits"])
        if W is not None:
            per_record = ref.expected(text, k, tables, mn, mx)
            assert np.array_equal(ref.record_sums(want["shared"], want["bin_first"]), per_record["shared"])
            binned = query_bins_ref.expected(text, k, tables, mn, mx, W)
            assert np.array_equal(want["hits"], binned["bin_hits"]) and np.array_equal(want["bin_first"], binned["bin_first"])
        else:
            assert np.array_equal(want["hits"], query_ref.expected(text, k, tables, mn, mx)["hits"])
    assert ref.expected(text, k, tables[:1], mn, mx)["shared"].shape == (4, 0)


# ------------------------------------------------------------------ qpairs -------------------------
def test_row_matrix_is_the_expansion_of_the_merger():
    rng = np.random.default_rng(3)
    for N in (1, 2, 3, 7, 16):
        hits = rng.integers(0, 2 ** 40, N).astype(np.uint64)
        shared = rng.integers(0, 2 ** 40, N * (N - 1) // 2).astype(np.uint64)
        pair = np.zeros((N, N), dtype=np.uint64)             # what pk_gram_expand takes: totals on the diagonal, shared above it
        pair[np.arange(N), np.arange(N)] = hits
        for p, (i, j) in enumerate(spectrum.pair_list(N)):
            pair[i, j] = shared[p]
        got = qpairs.row_matrix(hits, shared)
        assert got.dtype == np.uint64 and got.shape == (N, N, 3) and np.array_equal(got, _lib.gram_expand(pair))
    with pytest.raises(ValueError, match="pairs"):
        qpairs.row_matrix(np.zeros(3), np.zeros(2))


def test_jaccard_edge_cases():
    hits = np.array([[0, 0, 0], [5, 5, 0], [4, 2, 2 ** 40], [3, 3, 3]], dtype=np.uint64)
    shared = np.array([[0, 0, 0], [5, 0, 0], [1, 4, 2], [3, 3, 3]], dtype=np.uint64)      # pairs (0,1) (0,2) (1,2)
    d = qpairs.jaccard(hits, shared)
    assert d.dtype == np.float64 and d.shape == (4, 3)
    assert d[0].tolist() == [1.0, 1.0, 1.0]                  # a zero denominator
    assert d[1].tolist() == [0.0, 1.0, 1.0]                  # identical tables on this row: distance 0; nothing shared: 1
    assert d[2, 0] == 1 - 1 / 5 and d[2, 1] == 1 - 4 / 2 ** 40 and d[2, 2] == 1 - 2 / 2 ** 40
    assert d[3].tolist() == [0.0, 0.0, 0.0]
    assert qpairs.jaccard(np.zeros((2, 1), dtype=np.uint64), np.zeros((2, 0), dtype=np.uint64)).shape == (2, 0)


# ------------------------------------------------------------------ the group loop -----------------
def test_query_records_adds_shared_and_the_keyword_goes_only_when_set():
    k, text = 5, inputs.edge_fasta()
    dense = query_ref.random_tables(k, 17, seed=71)
    calls = []
    tables, stage, run = query_hooks(text, dense, calls)
    for N in (1, 4, 16):
        calls.clear()
        want = ref.expected(text, k, dense[:N], 2, 254)
        got = query.query_records("q.fa", tables[:N], 2, 254, hbm_budget=1 << 40, stage=stage, run=run, pairs=True)
        assert calls == [{"pairs": True}] and got["n_groups"] == 1
        assert got["shared"].dtype == np.uint64 and got["shared"].shape == (len(want["records"]), N * (N - 1) // 2)
        assert np.array_equal(got["shared"], want["shared"]) and "bin_shared" not in got
        assert got["pairs"].dtype == np.int32 and np.array_equal(got["pairs"], spectrum.pair_list(N))
        calls.clear()
        rows = ref.expected(text, k, dense[:N], 2, 254, W=3)
        got = query.query_records("q.fa", tables[:N], 2, 254, hbm_budget=1 << 40, stage=stage, run=run, bin_windows=3, pairs=True)
        assert calls == [{"bin_windows": 3, "pairs": True}]
        assert np.array_equal(got["bin_shared"], rows["shared"]) and np.array_equal(got["shared"], want["shared"])
    # without the option the hook is called as it always was, and the result carries none of the keys
    calls.clear()
    plain = query.query_records("q.fa", tables[:4], 2, 254, hbm_budget=1, stage=stage, run=run)
    assert calls == [{}] * 4 and not [key for key in plain if "shared" in key or "pairs" in key]
    # the refusals come before anything is staged or run
    calls.clear()
    with pytest.raises(ValueError, match="at most 16 tables"):
        query.query_records("q.fa", tables, 2, 254, hbm_budget=1 << 40, stage=stage, run=run, pairs=True)                      # N = 17
    with pytest.raises(ValueError, match="staged together"):
        query.query_records("q.fa", tables[:4], 2, 254, hbm_budget=2 * 4 ** k + 100, stage=stage, run=run, pairs=True)       # two groups
    with pytest.raises(ValueError, match="--pairs and --spectrum"):
        query.query_records("q.fa", tables[:4], 2, 254, hbm_budget=1 << 40, stage=stage, run=run, pairs=True, spectrum=True)
    assert calls == []


# ------------------------------------------------------------------ the writer ---------------------
def _result(W=None, coords=False, N=3):
    k, text = 5, inputs.edge_fasta()
    dense = query_ref.random_tables(k, N, seed=73)
    per_record = ref.expected(text, k, dense, 1, 255)
    plain = query_ref.expected(text, k, dense, 1, 255)
    names = query_ref.names(text, per_record["records"])
    res = {"names": [n + " \t" if i == 1 else n for i, n in enumerate(names)], "kmer_len": k, "min_count": 1, "max_count": 255,
           "seq_len": per_record["seq_len"], "n_valid": per_record["n_valid"], "hits": plain["hits"], "depth": plain["depth"],
           "shared": per_record["shared"], "pairs": per_record["pairs"]}
    if W is not None:
        rows = ref.expected(text, k, dense, 1, 255, W=W)
        binned = query_bins_ref.expected(text, k, dense, 1, 255, W)
        res.update(bin_windows=W, bin_first=rows["bin_first"], bin_shared=rows["shared"], bin_hits=binned["bin_hits"], bin_depth=binned["bin_depth"])
        if coords:
            B = int(rows["bin_first"][-1])
            res.update(bin_start=np.arange(B, dtype=np.uint64) * 3, bin_end=np.arange(B, dtype=np.uint64) * 3 + 9)
    return res, text, dense


def _data(tmp_path, N=3):
    return [{"pos": i, "index_file": tmp_path / f"t{i}.kin", "description_file": tmp_path / f"t{i}.kin.json",
             "header": {"kmer_len": 5, "project_name": f"t{'abc'[i]}", "input_file_name": f"{'abc'[i]}.fa"}} for i in range(N)]


@pytest.mark.parametrize("W,coords", [(None, False), (4, False), (4, True)])
def test_kmp_writer_and_qpairs(tmp_path, W, coords, capsys):
    res, text, dense = _result(W, coords)
    R = len(res["names"])
    rows = R if W is None else int(res["bin_first"][-1])
    proj = str(tmp_path / "proj")
    query.write_kmp(proj, res, "q.fa", _data(tmp_path), ["ta", "tb", "tc"])
    query.write_kmq(proj, res, "q.fa", _data(tmp_path), ["ta", "tb", "tc"])
    if W is not None:
        query.write_kmb(proj, res, "q.fa", _data(tmp_path), ["ta", "tb", "tc"])
    assert sorted(p.name for p in tmp_path.iterdir() if ".kmp" in p.name) == ["proj.kmp", "proj.kmp.json", "proj.kmp.tsv"]
    z = np.load(proj + ".kmp")
    more = ([] if W is None else ["bin_first", "bin_windows"]) + (["bin_start", "bin_end"] if coords else [])
    assert sorted(z.files) == sorted(["shared", "hits", "pairs", "n_valid", "seq_len", "kmer_len", "min_count", "max_count"] + more)
    assert z["shared"].dtype == np.uint64 and z["shared"].shape == (rows, 3) and np.array_equal(z["shared"], res["shared" if W is None else "bin_shared"])
    assert z["hits"].dtype == np.uint64 and np.array_equal(z["hits"], res["hits" if W is None else "bin_hits"]) and z["shared"].any()
    assert z["pairs"].dtype == np.int32 and z["pairs"].tolist() == [[0, 1], [0, 2], [1, 2]]
    assert z["n_valid"].dtype == z["seq_len"].dtype == np.uint64 and z["n_valid"].shape == (R,)
    assert (int(z["kmer_len"]), int(z["min_count"]), int(z["max_count"])) == (5, 1, 255)
    if W is not None:
        assert z["bin_first"].dtype == np.uint64 and np.array_equal(z["bin_first"], res["bin_first"]) and int(z["bin_windows"]) == W
    if coords:
        assert np.array_equal(z["bin_start"], res["bin_start"]) and np.array_equal(z["bin_end"], res["bin_end"])
    meta = json.load(open(proj + ".kmp.json"))
    src = json.load(open(proj + (".kmq.json" if W is None else ".kmb.json")))
    assert sorted(meta) == sorted(list(src) + ["n_pairs"]) and meta["n_pairs"] == 3
    assert {key: meta[key] for key in src} == src and ("coords" in meta) == coords
    lines = open(proj + ".kmp.tsv").read().split("\n")
    lead_src = open(proj + (".kmq.tsv" if W is None else ".kmb.tsv")).read().split("\n")
    lead = 3 if W is None else 6 if coords else 4
    assert lines[0].split("\t") == lead_src[0].split("\t")[:lead] + ["ta|tb", "ta|tc", "tb|tc"] and lines[-1] == "" and len(lines) == rows + 2
    assert ("start" in lines[0].split("\t")) == coords
    assert [ln.split("\t")[:lead] for ln in lines[1:-1]] == [ln.split("\t")[:lead] for ln in lead_src[1:-1]]
    assert np.array_equal(np.array([[int(v) for v in ln.split("\t")[lead:]] for ln in lines[1:-1]], dtype=np.uint64).reshape(-1, 3), z["shared"])

    # qpairs: load, one row as a .kma by index and by name, nothing overwritten
    kmp = qpairs.load(proj + ".kmp")
    assert kmp["meta"] == meta and kmp["kmer_len"] == 5 and np.array_equal(kmp["shared"], z["shared"])
    row = int(np.argmax(z["shared"].sum(axis=1)))
    qpairs.main([proj + ".kmp", str(tmp_path / "Q"), "--row", str(row)])
    assert "3 tables, 3 pairs" in capsys.readouterr().out
    got = np.load(tmp_path / "Q.001-255.kma")["matrix"]
    assert got.dtype == np.uint64 and np.array_equal(got, qpairs.row_matrix(z["hits"][row], z["shared"][row]))
    kma_meta = json.load(open(tmp_path / "Q.001-255.kma.json"))
    assert (kma_meta["min_count"], kma_meta["max_count"]) == (1, 255) and len(kma_meta["data"]) == 3
    names = [n.strip() for n in res["names"]]
    if W is None:
        r, b = row, None
    else:
        r = int(np.searchsorted(res["bin_first"].astype(np.int64), row, side="right")) - 1
        b = row - int(res["bin_first"][r])
    if names.index(names[r]) == r:                           # (a name that another record carries finds the first of them)
        qpairs.derive(proj + ".kmp", str(tmp_path / "N"), record=names[r], bin_index=b)
        assert np.array_equal(np.load(tmp_path / "N.001-255.kma")["matrix"], got)
    before = {p.name: p.read_bytes() for p in tmp_path.iterdir()}
    with pytest.raises(SystemExit) as e:
        qpairs.main([proj + ".kmp", str(tmp_path / "Q"), "--row", str(row)])
    assert e.value.code == 1 and "already exists" in capsys.readouterr().err
    for bad, match in (({"row": rows}, "rows"), ({}, "--row I or"), ({"row": 0, "record": "x"}, "--row I or"), ({"record": "no such record"}, "no record"),
                       ({"row": 0, "bin_index": 1}, "--bin goes with")):
        with pytest.raises(ValueError, match=match):
            qpairs.derive(proj + ".kmp", str(tmp_path / "X"), **bad)
    with pytest.raises(ValueError, match="does not exist"):
        qpairs.derive(str(tmp_path / "none.kmp"), str(tmp_path / "X"), row=0)
    # a query with --pairs overwrites none of the three, and checks before any work
    for ext in (".kmp", ".kmp.json", ".kmp.tsv"):
        only = tmp_path / ("only" + ext)
        only.write_bytes(b"")
        with pytest.raises(ValueError, match="already exists"):
            query.query(str(tmp_path / "only"), "q.fa", [tmp_path / "t0.kin"], pairs=True, **({} if W is None else {"bin_windows": W}))
        with pytest.raises(ValueError, match="query file does not exist"):      # without the option the file does not stop the run that early
            query.query(str(tmp_path / "only"), str(tmp_path / "none.fa"), [tmp_path / "t0.kin"])
        only.unlink()
    assert {p.name: p.read_bytes() for p in tmp_path.iterdir()} == before


def test_qpairs_runs_as_a_module_and_distance_reads_its_kma(tmp_path):
    res, _, _ = _result()
    query.write_kmp(str(tmp_path / "P"), res, "q.fa", _data(tmp_path), ["ta", "tb", "tc"])
    row = int(np.argmax(res["shared"].sum(axis=1)))
    run_py("-m", "pykmer_amd.qpairs", "P.kmp", "Q", "--row", str(row), cwd=str(tmp_path), env=env_with_root())
    m = distance.load(tmp_path / "Q.001-255.kma")
    assert m.shape[0] == 3 and np.array_equal(np.load(tmp_path / "Q.001-255.kma")["matrix"], qpairs.row_matrix(res["hits"][row], res["shared"][row]))


# ------------------------------------------------------------------ the CLI, stage and run substituted
def _cli(monkeypatch, tmp_path, n_tables, budget=1 << 40):
    k, text = 5, inputs.edge_fasta()
    dense = query_ref.random_tables(k, n_tables, seed=75)
    calls = []
    tables, stage, run = query_hooks(text, dense, calls)
    by_name = {}
    for i, t in enumerate(tables):
        kin = tmp_path / f"t{i}.kin"
        kin.write_bytes(b"")
        by_name[str(kin)] = t
    (tmp_path / "q.fa").write_bytes(text)
    monkeypatch.setattr(query, "load_header", lambda path, device=0: by_name[str(path)])
    monkeypatch.setattr(query, "stage_tables", stage)
    monkeypatch.setattr(query, "run_query", run)
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(budget))
    return text, dense, calls, [str(tmp_path / f"t{i}.kin") for i in range(n_tables)]


def test_cli_writes_the_kmp_files_beside_unchanged_kmq_and_kmb(monkeypatch, tmp_path, capsys):
    text, dense, calls, kins = _cli(monkeypatch, tmp_path, 3)
    before = {p.name for p in tmp_path.iterdir()}
    P, B, D = (str(tmp_path / n) for n in "PBD")
    query.main([P, str(tmp_path / "q.fa")] + kins + ["--pairs", "--min-count", "2"])
    assert capsys.readouterr().out.strip().splitlines()[-1].endswith("1 table group(s), 3 pairs")
    query.main([B, str(tmp_path / "q.fa")] + kins + ["--pairs", "--bin", "4", "--coords"])
    assert capsys.readouterr().out.strip().splitlines()[-1].endswith(" bins, 3 pairs")
    query.main([D, str(tmp_path / "q.fa")] + kins + ["--bin", "4", "--coords"])
    assert " pairs" not in capsys.readouterr().out.strip().splitlines()[-1]
    assert calls == [{"pairs": True}, {"bin_windows": 4, "coords": True, "pairs": True}, {"bin_windows": 4, "coords": True}]
    trio, kmb, kmp = ["kmq", "kmq.json", "kmq.tsv"], ["kmb", "kmb.json", "kmb.tsv"], ["kmp", "kmp.json", "kmp.tsv"]
    made = sorted(p.name for p in tmp_path.iterdir() if p.name not in before)
    assert made == sorted([f"P.{e}" for e in trio + kmp] + [f"B.{e}" for e in trio + kmb + kmp] + [f"D.{e}" for e in trio + kmb])
    for ext in trio + kmb:                                   # .kmq and .kmb are what they are without the option
        if ext.endswith(".json"):
            assert {**json.load(open(f"{B}.{ext}")), "project_name": D} == json.load(open(f"{D}.{ext}")), ext
        elif ext.endswith(".tsv"):
            assert open(f"{B}.{ext}", "rb").read() == open(f"{D}.{ext}", "rb").read(), ext
        else:
            zb, zd = np.load(f"{B}.{ext}"), np.load(f"{D}.{ext}")
            assert sorted(zb.files) == sorted(zd.files) and all(np.array_equal(zb[key], zd[key]) for key in zd.files), ext
    z = np.load(P + ".kmp")
    want = ref.expected(text, 5, dense, 2, 255)
    assert np.array_equal(z["shared"], want["shared"]) and np.array_equal(z["hits"], want["hits"]) and int(z["min_count"]) == 2
    zb = np.load(B + ".kmp")
    assert np.array_equal(zb["shared"], ref.expected(text, 5, dense, 1, 255, W=4)["shared"]) and "bin_start" in zb.files
    meta = json.load(open(B + ".kmp.json"))
    assert sorted(meta) == sorted(list(json.load(open(B + ".kmb.json"))) + ["n_pairs"]) and meta["coords"] is True and meta["bin_windows"] == 4
    assert open(P + ".kmp.tsv").readline().rstrip("\n").split("\t") == ["record", "seq_len", "n_valid", "ta|tb", "ta|tc", "tb|tc"]
    assert open(B + ".kmp.tsv").readline().rstrip("\n").split("\t")[:6] == ["record", "bin", "first_window", "n_windows", "start", "end"]


def test_cli_refusals_leave_no_file(monkeypatch, tmp_path, capsys):
    _, _, calls, kins = _cli(monkeypatch, tmp_path, 17)
    before = sorted(p.name for p in tmp_path.iterdir())
    for argv, match in ((kins[:3] + ["--pairs", "--spectrum"], "--spectrum"), (kins + ["--pairs"], "at most 16 tables")):
        with pytest.raises(SystemExit) as e:
            query.main([str(tmp_path / "p"), str(tmp_path / "q.fa")] + argv)
        err = capsys.readouterr().err
        assert e.value.code == 1 and err.startswith("error: ") and match in err
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(2 * 4 ** 5 + 100))            # two tables at a time
    with pytest.raises(SystemExit) as e:
        query.main([str(tmp_path / "p"), str(tmp_path / "q.fa")] + kins[:5] + ["--pairs"])
    err = capsys.readouterr().err
    assert e.value.code == 1 and err.startswith("error: ") and "staged together" in err
    assert calls == [] and sorted(p.name for p in tmp_path.iterdir()) == before
    query.main([str(tmp_path / "p"), str(tmp_path / "q.fa")] + kins[:5])       # the same budget without the option: three groups
    assert "3 table group(s)" in capsys.readouterr().out and calls == [{}] * 3


def test_parser_defaults():
    args = query.build_parser().parse_args(["p", "q.fa", "a.kin"])
    assert args.pairs is False and args.spectrum is False and args.bin_windows is None
    args = query.build_parser().parse_args(["p", "q.fa", "a.kin", "--pairs", "--bin", "100", "--coords"])
    assert args.pairs is True and args.bin_windows == 100 and args.coords is True
    args = qpairs.build_parser().parse_args(["P.kmp", "Q"])
    assert args.row is None and args.record is None and args.bin_index is None
    args = qpairs.build_parser().parse_args(["P.kmp", "Q", "--record", "chr1", "--bin", "3"])
    assert (args.record, args.bin_index) == ("chr1", 3)


# ------------------------------------------------------------------ the C ABI ----------------------
def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "pykmer_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+pk_query_set_pairs\s*\(\s*pk_indexer\s*\*\s*q\s*,\s*int\s+on\s*\)\s*;", code)
    assert re.search(r"int\s+pk_query_pairs\s*\(\s*pk_indexer\s*\*\s*q\s*,\s*uint64_t\s*\*\s*out\s*,\s*uint64_t\s+rows_cap\s*\)\s*;", code)
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines()}
    for name in ("pk_query_set_pairs", "pk_query_pairs"):
        assert name in _lib.EXPORTS and name in exported and hasattr(lib, name), name
    assert lib.pk_version() == 3
    assert callable(_lib.QueryIndexer.set_pairs) and callable(_lib.QueryIndexer.pairs)
    # argument checks that need no device
    one = np.zeros(1, dtype=np.uint64)
    assert lib.pk_query_set_pairs(None, 1) == _lib.PK_ERR_ARG
    assert lib.pk_query_pairs(None, one.ctypes.data, 1) == _lib.PK_ERR_ARG


def test_the_lds_accumulator_fits_beside_the_hit_tallies():
    """rows x P u32 beside acc_h / acc_d, at no more LDS than the spectrum instantiation takes (and so at its occupancy)."""
    src = open(os.path.join(ROOT, "pykmer_amd", "csrc", "kmer_query.hip")).read()
    rows = int(re.search(r"constexpr\s+uint32_t\s+QPAIR_ROWS\s*=\s*(\d+)\s*;", src).group(1))
    spec = int(re.search(r"constexpr\s+uint32_t\s+QSPEC_ROWS\s*=\s*(\d+)\s*;", src).group(1))
    assert query.MAX_PAIR_TABLES == 16
    assert rows * 120 * 4 <= spec * 256 * 4 and rows * 120 * 4 + 2 * 128 * 16 * 4 < 64 * 1024
