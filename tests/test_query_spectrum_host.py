"""CPU: the query's count spectra -- the yardstick (query_spectrum_ref), the helpers of pykmer_amd.qspectrum, the group loop of
query_records with a stubbed stage / run, the `.kmh` writer and the re-windowing tool.  No call here touches a GPU."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import inputs
import query_bins_ref
import query_ref
import query_spectrum_ref as ref
from host_support import query_hooks
from pykmer_amd import _lib, qspectrum, query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the yardstick ------------------
def test_spectrum_ref_agrees_with_the_hits_yardsticks():
    """Through the identities: every count window of the spectrum is what query_ref / query_bins_ref tally directly."""
    k = 9
    text, _ = query_ref.long_after_short(129, 1, ragged=True)
    tables = query_ref.random_tables(k, 3, 7)
    want = ref.expected(text, k, tables)
    assert want["spectrum"].shape == (len(want["records"]), 3, 256) and (want["n_valid"] == 0).any()
    for mn, mx in ((2, 254), (1, 255), (255, 255), (1, 1)):
        plain = query_ref.expected(text, k, tables, mn, mx)
        ref.check_identities(want["spectrum"], plain["n_valid"], plain["hits"], plain["depth"], mn, mx)
    for W in (1, 5, 1000):
        rows = ref.expected(text, k, tables, W)
        binned = query_bins_ref.expected(text, k, tables, 2, 254, W)
        assert np.array_equal(rows["bin_first"], binned["bin_first"])
        ref.check_identities(rows["spectrum"], binned["row_windows"], binned["bin_hits"], binned["bin_depth"], 2, 254)
        assert np.array_equal(ref.record_sums(rows["spectrum"], rows["bin_first"]), want["spectrum"])
    # the median against a literal one
    kmers, _ = __import__("oracle").kmer_list(text, k, records=True)
    bounds = np.concatenate([[0], np.cumsum(want["n_valid"])]).astype(np.int64)
    for r in (0, 1, 129, 130):
        for t in range(3):
            c = np.sort(tables[t][kmers[bounds[r]:bounds[r + 1]]])
            assert int(want["median"][r, t]) == (int(c[(c.size - 1) // 2]) if c.size else 0), (r, t)


# ------------------------------------------------------------------ the helpers --------------------
def _random_spectra(rng, n):
    spec = np.zeros((n, 256), dtype=np.uint64)
    for i in range(n):
        m = int(rng.integers(0, 40))
        counts = rng.choice(np.array([0, 0, 1, 2, 2, 2, 7, 254, 255]), m) if i % 2 else rng.integers(0, 256, m)
        np.add.at(spec[i], counts.astype(np.int64), 1)
    return spec


def test_window_and_median_from_spectrum_against_brute_force():
    rng = np.random.default_rng(5)
    hand = np.zeros((7, 256), dtype=np.uint64)
    hand[1, 0] = 1                                           # m = 1: the count itself
    hand[2, [3, 9]] = 1                                      # m = 2: the lower of the two
    hand[3, [3, 9]] = [2, 2]                                 # m = 4, ties: element 1 of 3 3 9 9
    hand[4, [0, 255]] = [1, 2]                               # m = 3: 255
    hand[5, [0, 255]] = [2, 2]                               # m = 4: 0
    hand[6, 255] = 2 ** 40                                   # counts beyond 32 bits
    got = qspectrum.median_from_spectrum(hand)
    assert got.dtype == np.uint8 and got.tolist() == [0, 0, 3, 3, 255, 0, 255]
    spec = np.concatenate([hand[:6], _random_spectra(rng, 200)]).reshape(103, 2, 256)
    assert (spec.sum(axis=-1) == 0).any() and (spec.sum(axis=-1) % 2 == 0).any()
    med = qspectrum.median_from_spectrum(spec)
    assert med.dtype == np.uint8 and med.shape == (103, 2) and np.array_equal(med, ref.median(spec))
    for mn, mx in ((1, 255), (2, 254), (255, 255), (1, 1), (7, 7)):
        hits, depth = qspectrum.window_from_spectrum(spec, mn, mx)
        want_h, want_d = ref.window(spec, mn, mx)
        assert hits.dtype == depth.dtype == np.uint64 and hits.shape == (103, 2)
        assert np.array_equal(hits, want_h) and np.array_equal(depth, want_d)
    big_h, big_d = qspectrum.window_from_spectrum(hand, 255, 255)
    assert int(big_h[6]) == 2 ** 40 and int(big_d[6]) == 255 * 2 ** 40                 # no detour through float
    for bad in ((0, 255), (1, 256), (5, 4)):
        with pytest.raises(ValueError, match="count window"):
            qspectrum.window_from_spectrum(spec, *bad)


# ------------------------------------------------------------------ the group loop -----------------
def test_table_groups_concatenate_spectra_and_the_keyword_goes_only_when_set():
    k, text = 5, inputs.edge_fasta()
    dense = query_ref.random_tables(k, 5, seed=61)
    calls = []
    tables, stage, run = query_hooks(text, dense, calls)
    per_record = ref.expected(text, k, dense)
    for budget, n_groups in ((1 << 40, 1), (2 * 4 ** k + 100, 3), (1, 5)):
        calls.clear()
        got = query.query_records("q.fa", tables, 2, 254, hbm_budget=budget, stage=stage, run=run, spectrum=True)
        assert got["n_groups"] == n_groups and calls == [{"spectrum": True}] * n_groups
        assert got["spectrum"].dtype == np.uint64 and np.array_equal(got["spectrum"], per_record["spectrum"])
        assert got["median"].dtype == np.uint8 and np.array_equal(got["median"], per_record["median"])
        assert "bin_spectrum" not in got and "bin_median" not in got
        ref.check_identities(got["spectrum"], got["n_valid"], got["hits"], got["depth"], 2, 254)
        calls.clear()
        W = 3
        rows = ref.expected(text, k, dense, W)
        got = query.query_records("q.fa", tables, 2, 254, hbm_budget=budget, stage=stage, run=run, bin_windows=W, spectrum=True)
        assert calls == [{"bin_windows": W, "spectrum": True}] * n_groups
        assert np.array_equal(got["bin_spectrum"], rows["spectrum"]) and np.array_equal(got["bin_median"], rows["median"])
        assert np.array_equal(got["spectrum"], per_record["spectrum"]) and np.array_equal(got["median"], per_record["median"])
        ref.check_identities(got["bin_spectrum"], rows["row_windows"], got["bin_hits"], got["bin_depth"], 2, 254)
    # without the option the hook is called as it always was, and the result carries none of the keys
    calls.clear()
    plain = query.query_records("q.fa", tables, 2, 254, hbm_budget=1, stage=stage, run=run)
    assert calls == [{}] * 5 and not [key for key in plain if "spectrum" in key or "median" in key]


def test_spectrum_record_sums():
    rng = np.random.default_rng(9)
    first = np.array([0, 3, 3, 4, 4], dtype=np.uint64)
    rows = rng.integers(0, 2 ** 40, (4, 2, 256)).astype(np.uint64)
    got = query.spectrum_record_sums(rows, first)
    assert got.dtype == np.uint64 and np.array_equal(got, ref.record_sums(rows, first))
    assert query.spectrum_record_sums(np.zeros((0, 2, 256), dtype=np.uint64), np.zeros(3, dtype=np.uint64)).shape == (2, 2, 256)


# ------------------------------------------------------------------ writers and qspectrum ----------
def _result(W=None):
    """A result as query_records returns it with spectrum=True (synthetic: the edge text against random tables)."""
    k, text = 5, inputs.edge_fasta()
    dense = query_ref.random_tables(k, 3, seed=63)
    per_record = ref.expected(text, k, dense)
    plain = query_ref.expected(text, k, dense, 1, 255)
    names = query_ref.names(text, per_record["records"])
    res = {"names": [n + " \t" if i == 1 else n for i, n in enumerate(names)], "kmer_len": k, "min_count": 1, "max_count": 255,
           "seq_len": per_record["seq_len"], "n_valid": per_record["n_valid"], "hits": plain["hits"], "depth": plain["depth"],
           "spectrum": per_record["spectrum"], "median": per_record["median"]}
    if W is not None:
        rows = ref.expected(text, k, dense, W)
        binned = query_bins_ref.expected(text, k, dense, 1, 255, W)
        res.update(bin_windows=W, bin_first=rows["bin_first"], bin_spectrum=rows["spectrum"], bin_median=rows["median"],
                   bin_hits=binned["bin_hits"], bin_depth=binned["bin_depth"])
    return res, text, dense


def _data(tmp_path):
    return [{"pos": i, "index_file": tmp_path / f"t{i}.kin", "description_file": tmp_path / f"t{i}.kin.json",
             "header": {"kmer_len": 5, "project_name": f"t{'abc'[i]}"}} for i in range(3)]


@pytest.mark.parametrize("W", [None, 4])
def test_kmh_writer_and_qspectrum(tmp_path, W, capsys):
    res, text, dense = _result(W)
    R = len(res["names"])
    rows = R if W is None else int(res["bin_first"][-1])
    proj = str(tmp_path / "proj")
    query.write_kmh(proj, res, "q.fa", _data(tmp_path), ["ta", "tb", "tc"])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["proj.kmh", "proj.kmh.json", "proj.kmh.tsv"]
    z = np.load(proj + ".kmh")
    assert sorted(z.files) == sorted(["spectrum", "median", "n_valid", "seq_len", "kmer_len"] + ([] if W is None else ["bin_first", "bin_windows"]))
    src = res["spectrum" if W is None else "bin_spectrum"]
    assert z["spectrum"].dtype == np.uint64 and z["spectrum"].shape == (rows, 3, 256) and np.array_equal(z["spectrum"], src)
    assert z["median"].dtype == np.uint8 and np.array_equal(z["median"], ref.median(src)) and z["median"].any()
    assert z["n_valid"].dtype == z["seq_len"].dtype == np.uint64 and z["n_valid"].shape == (R,) and int(z["kmer_len"]) == 5
    meta = json.load(open(proj + ".kmh.json"))
    assert sorted(meta) == sorted(["data", "kmer_len", "project_name", "query_file", "records"] + ([] if W is None else ["bin_windows", "n_bins"]))
    names = [n.strip() for n in res["names"]]
    assert meta["records"] == names and meta["query_file"] == "q.fa" and (W is None or (meta["bin_windows"], meta["n_bins"]) == (W, rows))
    lines = open(proj + ".kmh.tsv").read().split("\n")
    lead = ["record", "seq_len", "n_valid"] if W is None else ["record", "bin", "first_window", "n_windows"]
    assert lines[0].split("\t") == lead + ["ta", "tb", "tc"] and lines[-1] == "" and len(lines) == rows + 2
    cells = [ln.split("\t") for ln in lines[1:-1]]
    assert np.array_equal(np.array([[int(v) for v in c[len(lead):]] for c in cells], dtype=np.uint8).reshape(-1, 3), z["median"])
    if W is None:
        assert [c[:3] for c in cells] == [[n, str(int(s)), str(int(m))] for n, s, m in zip(names, res["seq_len"], res["n_valid"])]
    else:
        want = query_bins_ref.expected(text, 5, dense, 1, 255, W)
        assert [c[0] for c in cells] == [names[i] for i in want["row_record"]]
        assert [[int(v) for v in c[1:4]] for c in cells] == [[int(b), int(b) * W, int(n)] for b, n in zip(want["row_bin"], want["row_windows"])]

    # qspectrum at another window writes what the writers of a direct run write for that window's result
    mn, mx = 2, 200
    direct = dict(res, min_count=mn, max_count=mx)
    if W is None:
        plain = query_ref.expected(text, 5, dense, mn, mx)
    else:
        plain = query_bins_ref.expected(text, 5, dense, mn, mx, W)
        direct.update(bin_hits=plain["bin_hits"], bin_depth=plain["bin_depth"])
    direct.update(hits=plain["hits"], depth=plain["depth"])
    data = json.load(open(proj + ".kmh.json"))["data"]      # as a json file holds it: paths are strings
    query.write_kmq(str(tmp_path / "D"), direct, "q.fa", data, ["ta", "tb", "tc"])
    if W is not None:
        query.write_kmb(str(tmp_path / "D"), direct, "q.fa", data, ["ta", "tb", "tc"])
    qspectrum.main([proj + ".kmh", str(tmp_path / "S"), "--min-count", str(mn), "--max-count", str(mx)])
    trio = ["kmq", "kmq.json", "kmq.tsv"] + ([] if W is None else ["kmb", "kmb.json", "kmb.tsv"])
    assert sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("S.")) == sorted(f"S.{e}" for e in trio)
    for ext in trio:
        if ext.endswith(".json"):
            assert {**json.load(open(tmp_path / f"S.{ext}")), "project_name": str(tmp_path / "D")} == json.load(open(tmp_path / f"D.{ext}")), ext
        elif ext.endswith(".tsv"):
            assert (tmp_path / f"S.{ext}").read_bytes() == (tmp_path / f"D.{ext}").read_bytes(), ext
        else:
            zs, zd = np.load(tmp_path / f"S.{ext}"), np.load(tmp_path / f"D.{ext}")
            assert sorted(zs.files) == sorted(zd.files)
            for key in zd.files:
                assert zs[key].dtype == zd[key].dtype and np.array_equal(zs[key], zd[key]), (ext, key)
    assert "coords" not in json.load(open(tmp_path / "S.kmq.json"))

    # nothing is overwritten: by qspectrum, and by a query with --spectrum
    before = {p.name: p.read_bytes() for p in tmp_path.iterdir()}
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        qspectrum.main([proj + ".kmh", str(tmp_path / "S")])
    assert e.value.code == 1 and capsys.readouterr().err.startswith("error: ")
    for ext in trio:
        only = tmp_path / f"only.{ext}"
        only.write_bytes(b"")
        with pytest.raises(ValueError, match="already exists"):
            qspectrum.derive(proj + ".kmh", str(tmp_path / "only"))
        only.unlink()
    for ext in (".kmh", ".kmh.json", ".kmh.tsv"):
        only = tmp_path / ("only" + ext)
        only.write_bytes(b"")
        with pytest.raises(ValueError, match="already exists"):
            query.query(str(tmp_path / "only"), "q.fa", [tmp_path / "t0.kin"], spectrum=True, **({} if W is None else {"bin_windows": W}))
        with pytest.raises(ValueError, match="query file does not exist"):      # without the option the file does not stop the run that early
            query.query(str(tmp_path / "only"), str(tmp_path / "none.fa"), [tmp_path / "t0.kin"])
        only.unlink()
    with pytest.raises(ValueError, match="count window"):
        qspectrum.derive(proj + ".kmh", str(tmp_path / "X"), 0, 255)
    with pytest.raises(ValueError, match="does not exist"):
        qspectrum.derive(str(tmp_path / "none.kmh"), str(tmp_path / "X"))
    assert {p.name: p.read_bytes() for p in tmp_path.iterdir()} == before


def test_qspectrum_runs_as_a_module_without_a_device(tmp_path):
    res, _, _ = _result()
    query.write_kmh(str(tmp_path / "P"), res, "q.fa", _data(tmp_path), ["ta", "tb", "tc"])
    code = ("import sys, runpy; sys.argv = ['qspectrum', 'P.kmh', 'Q', '--min-count', '3']; "
            "import pykmer_amd._lib as L; L.load = None; runpy.run_module('pykmer_amd.qspectrum', run_name='__main__')")
    r = subprocess.run([__import__("sys").executable, "-c", code], cwd=str(tmp_path), capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 0, r.stderr[-2000:]
    assert int(np.load(tmp_path / "Q.kmq")["min_count"]) == 3 and "count window 3-255" in r.stdout


def test_cli_option():
    args = query.build_parser().parse_args(["p", "q.fa", "a.kin"])
    assert args.spectrum is False
    args = query.build_parser().parse_args(["p", "q.fa", "a.kin", "--spectrum", "--bin", "100"])
    assert args.spectrum is True and args.bin_windows == 100


# ------------------------------------------------------------------ the C ABI ----------------------
def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "pykmer_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+pk_query_set_spectrum\s*\(\s*pk_indexer\s*\*\s*q\s*,\s*int\s+on\s*\)\s*;", code)
    assert re.search(r"int\s+pk_query_spectrum\s*\(\s*pk_indexer\s*\*\s*q\s*,\s*uint64_t\s*\*\s*out\s*,\s*uint64_t\s+rows_cap\s*\)\s*;", code)
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines()}
    for name in ("pk_query_set_spectrum", "pk_query_spectrum"):
        assert name in _lib.EXPORTS and name in exported and hasattr(lib, name), name
    assert lib.pk_version() == 3
    # argument checks that need no device
    one = np.zeros(1, dtype=np.uint64)
    assert lib.pk_query_set_spectrum(None, 1) == _lib.PK_ERR_ARG
    assert lib.pk_query_spectrum(None, one.ctypes.data, 1) == _lib.PK_ERR_ARG


def test_the_gpu_tests_mirror_the_kernel_constant():
    """tests/test_gpu_query_spectrum.py places its long record around the last LDS-resident row."""
    src = open(os.path.join(ROOT, "pykmer_amd", "csrc", "kmer_query.hip")).read()
    rows = int(re.search(r"constexpr\s+uint32_t\s+QSPEC_ROWS\s*=\s*(\d+)\s*;", src).group(1))
    gpu_test = open(os.path.join(ROOT, "tests", "test_gpu_query_spectrum.py")).read()
    assert int(re.search(r"^QSPEC_ROWS = (\d+)", gpu_test, flags=re.M).group(1)) == rows
    assert rows * 256 * 4 + 2 * 128 * 16 * 4 < 64 * 1024     # the histogram beside the hit tallies, within a workgroup's static LDS
