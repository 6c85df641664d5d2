"""CPU: base coordinates of binned query hits -- the yardstick (query_coords_ref) against the oracle and against what follows
from the definition, the refusals of `--coords` without `--bin`, and the `.kmb` writers.  No call here touches a GPU."""
import json

import numpy as np
import pytest

import oracle
import query_bins_ref
import query_coords_inputs as qci
import query_coords_ref
import query_ref
from fastq_ref import fastq_to_fasta
from host_support import query_hooks
from pykmer_amd import query


@pytest.mark.parametrize("case", qci.all_texts(), ids=lambda c: c[0])
def test_ref_agrees_with_the_oracle(case):
    """The walker of query_coords_ref and the oracle's were written separately: same records, seq_len and windows per
    record on every text of the GPU tests."""
    _, text, k, fmt = case
    seq_len, n_windows, starts = query_coords_ref.window_starts(text, k, fmt)
    _, info = oracle.kmer_list(fastq_to_fasta(text) if fmt == "fastq" else text, k, records=True)
    recs = info["records"]
    assert len(recs) == seq_len.size == n_windows.size and len(recs) >= 1
    assert np.array_equal(recs["seq_len"].astype(np.uint64), seq_len)
    assert np.array_equal(recs["n_valid_kmers"].astype(np.uint64), n_windows)
    assert starts.size == int(n_windows.sum()) == info["num_kmers"]


@pytest.mark.parametrize("case", qci.all_texts(), ids=lambda c: c[0])
def test_consequences_of_the_definition(case):
    name, text, k, fmt = case
    tables = [query_ref.SparseTable(np.zeros(0, dtype=np.uint64))]        # coordinates do not depend on the tables
    for W in (1, 5, 100, 5000, 10 ** 9):
        want = query_coords_ref.expected(text, k, tables, 1, 255, W, fmt)
        assert want["bin_start"].dtype == want["bin_end"].dtype == np.uint64
        assert want["bin_start"].shape == want["bin_end"].shape == (int(want["bin_first"][-1]),)
        query_coords_ref.check_consequences(want, k, W, gap_free=name.startswith(("one_record", "many", "short_reads")))


def test_window_starts_of_the_gapped_record():
    """On the one-record A/C/G/T/N text the starts are those of query_ref.straddling_windows, and a row is as long as its
    windows and k - 1 exactly when no N lies inside it."""
    for k in (5, 9):
        text, runs = qci.gapped(k)
        _, n_windows, starts = query_coords_ref.window_starts(text, k)
        start = query_ref.straddling_windows(text, k)[0]
        assert n_windows.size == 1 and np.array_equal(starts.astype(np.int64), start)
        seq = np.frombuffer(text[qci.GAP_HEAD:].replace(b"\n", b""), dtype=np.uint8)
        n_before = np.concatenate([[0], np.cumsum(seq == ord("N"))])
        some_gap = some_plain = False
        for W in (1, 5, 100, 5000):
            b_start, b_end = (a.astype(np.int64) for a in query_coords_ref.bin_coords(n_windows, starts, k, W))
            rows = query_bins_ref.bin_bounds(n_windows, W)
            tight = b_end - b_start == (rows[2] - rows[1]) + k - 1
            clean = n_before[b_end] == n_before[b_start]
            assert np.array_equal(tight, clean)
            some_gap |= bool((~clean).any())
            some_plain |= bool(clean.any())
        assert some_gap and some_plain
        # where the runs lie: the text offsets the GPU cases are about
        offs = [(qci.base_offset(qci.GAP_HEAD, lo), qci.base_offset(qci.GAP_HEAD, lo + n - 1)) for lo, n in runs]
        assert any(a // qci.PIECE == b // qci.PIECE for a, b in offs) and any(a // qci.PIECE != b // qci.PIECE for a, b in offs)
        assert {b // qci.CHUNK for a, b in offs if a // qci.CHUNK != b // qci.CHUNK} >= {2, 3, 4, 5, 6, 7}
        assert offs[0][0] == qci.GAP_HEAD and offs[-1][1] == len(text) - 2


def test_blank_text_positions_by_hand():
    """A small text worked out by hand: interior blanks hold positions, leading and trailing ones do not."""
    text = b"ACGTACGT\n>a\n  ACG T\t\nAC  GTAC \r\n\n>b\n>c\nAC\rGTN\nACGTA\n"
    seq_len, n_windows, starts = query_coords_ref.window_starts(text, 3)
    # a: "ACG T" + "AC  GTAC" = positions 0-4, 5-12; windows ACG (0), TAC across the line end (4), GTA (9), TAC (10).
    # b: empty.  c: "AC" "GTN" "ACGTA" = ACGTNACGTA
    assert list(seq_len) == [13, 0, 10] and list(n_windows) == [4, 0, 5]
    assert list(starts) == [0, 4, 9, 10, 0, 1, 5, 6, 7]
    b_start, b_end = query_coords_ref.bin_coords(n_windows, starts, 3, 2)
    assert list(b_start) == [0, 9, 0, 5, 7] and list(b_end) == [7, 13, 4, 9, 10]


def test_cli_refuses_coords_without_bins(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        query.main([str(tmp_path / "p"), str(tmp_path / "q.fa"), str(tmp_path / "a.kin"), "--coords"])
    assert e.value.code == 1
    assert capsys.readouterr().err.startswith("error: ")
    assert not list(tmp_path.iterdir())
    args = query.build_parser().parse_args(["p", "q.fa", "a.kin", "--bin", "50", "--coords"])
    assert args.coords is True and args.bin_windows == 50
    assert query.build_parser().parse_args(["p", "q.fa", "a.kin", "--bin", "50"]).coords is False


def test_query_records_passes_coords_through_and_refuses_them_without_bins():
    k, W, text = 5, 3, qci.many_records(127)
    dense = query_ref.random_tables(k, 3, seed=64)
    calls = []
    tables, stage, run = query_hooks(text, dense, calls)
    with pytest.raises(ValueError, match="coords"):
        query.query_records("q.fa", tables, 1, 255, stage=stage, run=run, coords=True)
    with pytest.raises(ValueError, match="coords"):
        query.query("p", "q.fa", ["a.kin"], coords=True)
    assert not calls
    want = query_coords_ref.expected(text, k, dense, 1, 255, W)
    got = query.query_records("q.fa", tables, 1, 255, hbm_budget=1, stage=stage, run=run, bin_windows=W, coords=True)
    assert calls == [{"bin_windows": W, "coords": True}] * 3 and got["n_groups"] == 3
    for key in ("bin_start", "bin_end", "bin_hits", "bin_first"):
        assert got[key].dtype == np.uint64 and np.array_equal(got[key], want[key]), key
    calls.clear()
    got = query.query_records("q.fa", tables, 1, 255, hbm_budget=1, stage=stage, run=run, bin_windows=W)
    assert calls == [{"bin_windows": W}] * 3 and "bin_start" not in got and "bin_end" not in got and "coords_s" not in got


def test_kmb_writers_with_and_without_coords(tmp_path):
    k, W, text = 5, 4, qci.blanks()
    dense = query_ref.random_tables(k, 2, seed=65)
    want = query_coords_ref.expected(text, k, dense, 1, 255, W)
    base = {key: want[key] for key in ("seq_len", "n_valid", "hits", "depth", "bin_hits", "bin_depth", "bin_first")}
    base.update(names=query_ref.names(text, want["records"]), kmer_len=k, min_count=1, max_count=255, bin_windows=W)
    B = int(want["bin_first"][-1])
    query.write_kmb(str(tmp_path / "plain"), base, "q.fa", [], ["ta", "tb"])
    query.write_kmb(str(tmp_path / "co"), {**base, "bin_start": want["bin_start"], "bin_end": want["bin_end"]}, "q.fa", [], ["ta", "tb"])
    zp, zc = np.load(tmp_path / "plain.kmb"), np.load(tmp_path / "co.kmb")
    assert sorted(zp.files) == ["bin_first", "bin_windows", "depth", "hits", "kmer_len", "max_count", "min_count", "n_valid", "seq_len"]
    assert sorted(zc.files) == sorted(zp.files + ["bin_start", "bin_end"])
    for key in zp.files:
        assert np.array_equal(zp[key], zc[key]), key
    for key in ("bin_start", "bin_end"):
        assert zc[key].dtype == np.uint64 and zc[key].shape == (B,) and np.array_equal(zc[key], want[key])
    mp, mc = json.loads((tmp_path / "plain.kmb.json").read_text()), json.loads((tmp_path / "co.kmb.json").read_text())
    assert "coords" not in mp and mc["coords"] is True
    assert {**mc, "project_name": mp["project_name"]} == {**mp, "coords": True}
    lp, lc = ((tmp_path / f"{p}.kmb.tsv").read_text().split("\n") for p in ("plain", "co"))
    assert lp[0].split("\t") == ["record", "bin", "first_window", "n_windows", "ta", "tb"]
    assert lc[0].split("\t") == ["record", "bin", "first_window", "n_windows", "start", "end", "ta", "tb"]
    assert len(lp) == len(lc) == B + 2
    for i, (a, b) in enumerate(zip(lp[1:-1], lc[1:-1])):
        a, b = a.split("\t"), b.split("\t")
        assert b[:4] == a[:4] and b[6:] == a[4:] and [int(b[4]), int(b[5])] == [int(want["bin_start"][i]), int(want["bin_end"][i])]
