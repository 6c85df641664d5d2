"""CPU: binned query hits -- the yardstick (query_bins_ref), the validation of W, the record sums, the group loop and the
three `.kmb` writers.  No call here touches a GPU: staging and streaming are stood in for by query_bins_ref."""
import json
import types

import numpy as np
import pytest

import inputs
import query_bins_ref
import query_ref
from oracle import pyoracle
from host_support import query_hooks
from pykmer_amd import query


def test_bins_ref_agrees_with_a_literal_restatement():
    """Pins the yardstick: per record, cut the windows the reference's gen_kmers yields into lists of W and look each up."""
    k, text = 5, inputs.edge_fasta()
    tables = query_ref.random_tables(k, 2, seed=60)
    recs = list(pyoracle.records(text.decode("utf-8")))
    for W in (1, 2, 3, 7, 10 ** 9):
        for mn, mx in ((1, 255), (2, 254)):
            want = query_bins_ref.expected(text, k, tables, mn, mx, W)
            plain = query_ref.expected(text, k, tables, mn, mx)
            for key in ("hits", "depth", "n_valid", "seq_len"):
                assert np.array_equal(want[key], plain[key]), key
            rows_h, rows_d, first, some_empty, some_partial = [], [], [0], False, False
            for name, seq, seq_len in recs:
                canon = [min(f, v) for _, f, v in pyoracle.windows(seq, k)]
                some_empty |= not canon
                for j in range(0, len(canon), W):
                    piece = canon[j:j + W]
                    some_partial |= len(piece) < W
                    c = [[int(table[a]) for a in piece] for table in tables]
                    rows_h.append([sum(1 for v in ct if mn <= v <= mx) for ct in c])
                    rows_d.append([sum(v for v in ct if mn <= v <= mx) for ct in c])
                first.append(len(rows_h))
            assert some_empty and (some_partial or W == 1)
            assert np.array_equal(want["bin_first"], np.array(first, dtype=np.uint64)) and want["bin_first"].dtype == np.uint64
            assert np.array_equal(want["bin_hits"], np.array(rows_h, dtype=np.uint64).reshape(-1, 2))
            assert np.array_equal(want["bin_depth"], np.array(rows_d, dtype=np.uint64).reshape(-1, 2))


def test_validation_of_the_bin_size():
    for good in (1, 7, np.int64(500), 2 ** 64 - 1):
        assert query.validate_bins(good) == int(good)
    for bad in (0, -1, -500, 2 ** 64, 2.0, "7", True, None):
        with pytest.raises(ValueError, match="bin size"):
            query.validate_bins(bad)
    a = types.SimpleNamespace(kmer_len=9, index_file="a.kin", data_size=4 ** 9)
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError, match="bin size"):            # before anything is staged or streamed
            query.query_records("q.fa", [a], 1, 255, bin_windows=bad, stage=None, run=None)


def test_cli_refuses_a_bin_size_below_one(tmp_path, capsys):
    for bad in ("0", "-4"):
        with pytest.raises(SystemExit) as e:
            query.main([str(tmp_path / "p"), str(tmp_path / "q.fa"), str(tmp_path / "a.kin"), "--bin", bad])
        assert e.value.code == 1
        assert capsys.readouterr().err.startswith("error: ")
    assert not list(tmp_path.iterdir())
    assert query.build_parser().parse_args(["p", "q.fa", "a.kin"]).bin_windows is None
    assert query.build_parser().parse_args(["p", "q.fa", "a.kin", "--bin", "500"]).bin_windows == 500


def test_record_sums_from_rows():
    rng = np.random.default_rng(7)
    for n_rows in ([3, 0, 0, 2, 1, 0], [0, 0, 4], [0], [5], [1, 0], [0, 0], []):     # records without a row; the last one empty
        first = np.concatenate([[0], np.cumsum(n_rows)]).astype(np.uint64)
        rows = rng.integers(0, 2 ** 40, (int(first[-1]), 3)).astype(np.uint64)
        got = query.record_sums(rows, first)
        assert got.dtype == np.uint64 and got.shape == (len(n_rows), 3)
        for r, n in enumerate(n_rows):
            assert np.array_equal(got[r], rows[int(first[r]):int(first[r]) + n].sum(axis=0, dtype=np.uint64)), (n_rows, r)
    big = np.full((2, 1), 2 ** 63, dtype=np.uint64)                                   # no detour through float or int64
    assert int(query.record_sums(big, [0, 1, 2])[1, 0]) == 2 ** 63
    with pytest.raises(AssertionError, match="bin_first"):
        query.record_sums(np.zeros((3, 1), dtype=np.uint64), [0, 2])


def test_table_groups_concatenate_bin_columns():
    k, W, text = 5, 3, inputs.edge_fasta()
    dense = query_ref.random_tables(k, 5, seed=61)
    calls = []
    tables, stage, run = query_hooks(text, dense, calls)
    want = query_bins_ref.expected(text, k, dense, 2, 254, W)
    for budget, n_groups in ((1 << 40, 1), (2 * 4 ** k + 100, 3), (1, 5)):
        calls.clear()
        got = query.query_records("q.fa", tables, 2, 254, hbm_budget=budget, stage=stage, run=run, bin_windows=W)
        assert got["n_groups"] == n_groups and calls == [{"bin_windows": W}] * n_groups and got["bin_windows"] == W
        assert got["bin_hits"].shape == (int(want["bin_first"][-1]), 5) and got["bin_first"].shape == (len(want["records"]) + 1,)
        for key in ("hits", "depth", "n_valid", "seq_len", "bin_hits", "bin_depth", "bin_first"):
            assert got[key].dtype == np.uint64 and np.array_equal(got[key], want[key]), key
    # without bin_windows the hook is called as it always was, and the result carries no bin key
    calls.clear()
    plain = query.query_records("q.fa", tables, 2, 254, hbm_budget=1, stage=stage, run=run)
    assert calls == [{}] * 5 and not [key for key in plain if key.startswith("bin_")]
    assert np.array_equal(plain["hits"], want["hits"])


def test_groups_that_disagree_on_bin_first_are_refused():
    k, text = 5, inputs.edge_fasta()
    dense = query_ref.random_tables(k, 2, seed=62)
    calls = []
    tables, stage, run = query_hooks(text, dense, calls)

    def drifting(*args, **kw):
        out = run(*args, **kw)
        if len(calls) == 2:                                  # the second group sees other bins
            out["bin_first"] = out["bin_first"].copy()
            out["bin_first"][1] += np.uint64(1)
        return out

    with pytest.raises(AssertionError, match="bins changed"):
        query.query_records("q.fa", tables, 1, 255, hbm_budget=1, stage=stage, run=drifting, bin_windows=4)


def _binned_result(W=4):
    k, text = 5, inputs.edge_fasta()
    dense = query_ref.random_tables(k, 3, seed=63)
    want = query_bins_ref.expected(text, k, dense, 2, 200, W)
    res = {key: want[key] for key in ("seq_len", "n_valid", "hits", "depth", "bin_hits", "bin_depth", "bin_first")}
    names = query_ref.names(text, want["records"])
    res.update(names=[n + " \t" if i == 1 else n for i, n in enumerate(names)], kmer_len=k, min_count=2, max_count=200, bin_windows=W)
    return res, want


def test_kmb_writers(tmp_path):
    W = 4
    res, want = _binned_result(W)
    R, B = len(res["names"]), int(want["bin_first"][-1])
    assert B > R > 3 and (want["n_valid"] == 0).any() and (want["row_windows"] < W).any()
    proj = str(tmp_path / "proj")
    data = [{"pos": i, "index_file": tmp_path / f"t{i}.kin", "description_file": tmp_path / f"t{i}.kin.json", "header": {"kmer_len": 5}}
            for i in range(3)]
    query.write_kmb(proj, res, "q.fa", data, ["ta", "tb", "tc"])
    assert not list(tmp_path.glob("*.tmp"))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["proj.kmb", "proj.kmb.json", "proj.kmb.tsv"]
    z = np.load(proj + ".kmb")
    assert sorted(z.files) == ["bin_first", "bin_windows", "depth", "hits", "kmer_len", "max_count", "min_count", "n_valid", "seq_len"]
    for key, src, shape in (("hits", "bin_hits", (B, 3)), ("depth", "bin_depth", (B, 3)), ("bin_first", "bin_first", (R + 1,)),
                            ("n_valid", "n_valid", (R,)), ("seq_len", "seq_len", (R,))):
        assert z[key].dtype == np.uint64 and z[key].shape == shape and np.array_equal(z[key], want[src]), key
    assert (int(z["bin_windows"]), int(z["kmer_len"]), int(z["min_count"]), int(z["max_count"])) == (W, 5, 2, 200)
    with open(proj + ".kmb.json") as fh:
        meta = json.load(fh)
    assert sorted(meta) == ["bin_windows", "data", "kmer_len", "max_count", "min_count", "n_bins", "project_name", "query_file", "records"]
    names = [n.strip() for n in res["names"]]
    assert meta["records"] == names and meta["bin_windows"] == W and meta["n_bins"] == B and meta["query_file"] == "q.fa"
    assert [d["pos"] for d in meta["data"]] == [0, 1, 2] and meta["data"][1]["index_file"] == str(tmp_path / "t1.kin")
    lines = open(proj + ".kmb.tsv").read().split("\n")
    assert lines[0] == "record\tbin\tfirst_window\tn_windows\tta\ttb\ttc" and lines[-1] == "" and len(lines) == B + 2
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert [r[0] for r in rows] == [names[i] for i in want["row_record"]]
    assert [int(r[1]) for r in rows] == list(want["row_bin"]) and [int(r[2]) for r in rows] == [int(b) * W for b in want["row_bin"]]
    assert [int(r[3]) for r in rows] == list(want["row_windows"])
    assert np.array_equal(np.array([[int(v) for v in r[4:]] for r in rows], dtype=np.uint64), want["bin_hits"])
    # none of the six files is overwritten: a .kmb file alone stops a binned run, and does not stop a plain one that early
    for ext in (".kmb", ".kmb.json", ".kmb.tsv"):
        only = tmp_path / ("only" + ext)
        only.write_bytes(b"")
        with pytest.raises(ValueError, match="already exists"):
            query.query(str(tmp_path / "only"), "q.fa", [tmp_path / "t0.kin"], bin_windows=W)
        with pytest.raises(ValueError, match="query file does not exist"):
            query.query(str(tmp_path / "only"), str(tmp_path / "none.fa"), [tmp_path / "t0.kin"])
        only.unlink()
    (tmp_path / "other.kmq.tsv").write_bytes(b"")
    with pytest.raises(ValueError, match="already exists"):
        query.query(str(tmp_path / "other"), "q.fa", [tmp_path / "t0.kin"], bin_windows=W)


def test_kmb_of_a_query_without_windows(tmp_path):
    res = {"names": ["a", "b"], "seq_len": np.array([3, 0], dtype=np.uint64), "n_valid": np.zeros(2, dtype=np.uint64),
           "bin_hits": np.zeros((0, 2), dtype=np.uint64), "bin_depth": np.zeros((0, 2), dtype=np.uint64),
           "bin_first": np.zeros(3, dtype=np.uint64), "kmer_len": 5, "min_count": 1, "max_count": 255, "bin_windows": 10}
    proj = str(tmp_path / "empty")
    query.write_kmb(proj, res, "q.fa", [], ["ta", "tb"])
    z = np.load(proj + ".kmb")
    assert z["hits"].shape == (0, 2) and z["hits"].dtype == np.uint64 and list(z["bin_first"]) == [0, 0, 0]
    assert open(proj + ".kmb.tsv").read() == "record\tbin\tfirst_window\tn_windows\tta\ttb\n"
