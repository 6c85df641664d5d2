"""Unitigs without a GPU: the reference module against hand-written cases and its own invariants, the CLI's refusals, the
writers through the stage / run hooks, n50, and the C-ABI surface."""
import ctypes
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import unitig_inputs as ui
import unitig_ref as ref
from host_support import ROOT, write_kin
from pykmer_amd import _lib, unitigs

UNITIG_SYMBOLS = ("pk_unitig_create", "pk_unitig_build", "pk_unitig_rows", "pk_unitig_text", "pk_unitig_timings", "pk_unitig_destroy")


def _of(seqs, k, **kw):
    counts = {}
    for s in seqs:
        for x in ref.kmers_of(s, k):
            counts[x] = counts.get(x, 0) + 1
    got = ref.expected(counts, k, **kw)
    ref.check_invariants(got, kw.get("min_kmers", 1))
    return got


def _rows(got):
    return list(zip(ref.texts(got), got["n_kmers"].tolist(), got["circular"].tolist()))


# ------------------------------------------------------------------ the reference: hand cases -----
def test_literal_cases():
    assert _rows(_of(["ACACACAC"], 5)) == [("ACACAC", 2, 1)]                       # one circular unitig, n = 2
    got = _of(["AAAAATTTTT"], 5)
    assert _rows(got) == [("AAAAA", 1, 0), ("AAAATT", 2, 0)]                       # AAAAA is a self-loop end
    assert got["depth"].tolist() == [2, 4] and got["first_addr"].tolist() == [0, ref.encode("AAAAT")]     # AAAAA = rc(TTTTT): counted twice
    assert "self_loop" in ui.features(got["graph"])


def test_snp_bubble_and_y_branch():
    k = 9
    rng, seen = random.Random(9), set()
    left, right = ui.distinct_sequence(rng, 20, k, seen), ui.distinct_sequence(rng, 20, k, seen)
    a, b = left + "A" + right, left + "C" + right
    got = _of([a, b], k)
    sizes = sorted(got["n_kmers"].tolist())
    assert sizes == [9, 9, 12, 12] and got["n_circular"] == 0 and got["n_branching"] == 2      # the flanks end at the fork nodes; the alleles are 9 nodes each
    want = {a[20 - k + 1:20 + k], b[20 - k + 1:20 + k]}
    alleles = [t for t, n in zip(ref.texts(got), got["n_kmers"]) if n == 9]
    assert {t if t in want else _rc_text(t) for t in alleles} == want
    # a Y: one stem, two arms
    stem, arm1, arm2 = (ui.distinct_sequence(rng, 25, k, seen) for _ in range(3))
    got = _of([stem + arm1, stem[-(k - 1):] + arm2], k)
    assert got["n_branching"] == 1 and len(got["n_kmers"]) >= 3 and got["n_nodes"] == int(got["n_kmers"].sum())
    branch = ref.canon(ref.encode(stem[-k:]), k)
    assert got["graph"].branching(branch) and any(branch in (ref.canon(p[0], k), ref.canon(p[-1], k)) for p in got["paths"])


def _rc_text(text):
    return text[::-1].translate(str.maketrans("ACGT", "TGCA"))


def test_hairpin_end():
    """ACGTT + its continuation: o = AACGT -> ACGTT = rc(AACGT), an edge o -> rc(o).  It counts in the degrees and is never
    compacted, so the path ends at the hairpin node."""
    k = 5
    text = "CCTGAACGT"                                       # ... AACGT, whose successor ACGTT is its own reverse complement's node
    got = _of([text], k)
    o = ref.encode("AACGT")
    g = got["graph"]
    assert ref.rc(o, k) == ref.encode("ACGTT") and ref.rc(o, k) in g.out(o) and "hairpin" in ui.features(g)
    assert g.succ(o) is None and not g.compactable(o, ref.rc(o, k))
    assert len(got["n_kmers"]) == 1 and got["n_kmers"].tolist() == [5] and ref.texts(got)[0] in (text, _rc_text(text))


@pytest.mark.parametrize("k", [3, 5, 7])
def test_invariants_on_random_sets(k):
    rng = random.Random(70 + k)
    for d in (0.02, 0.1, 0.3, 0.6, 1.0):
        counts = {x: 1 + x % 9 for x in range(4 ** k) if x == ref.canon(x, k) and (d == 1.0 or rng.random() < d)}
        got = ref.expected(counts, k)
        ref.check_invariants(got)
        g = got["graph"]
        for o in list(g.oriented)[:200]:                     # compactable edges are symmetric
            t = g.succ(o)
            if t is not None:
                assert g.succ(ref.rc(t, k)) == ref.rc(o, k)
        for M in (2, 3):
            cut = ref.expected(counts, k, min_kmers=M)
            ref.check_invariants(cut, M)
            keep = got["n_kmers"] >= M
            assert np.array_equal(cut["first_addr"], got["first_addr"][keep]) and cut["n_short"] == int((~keep).sum())
            assert cut["nodes_short"] == int(got["n_kmers"][~keep].sum())


def test_window_selects_the_nodes():
    counts = {x: v for x, v in zip(ref.kmers_of("ACGGTCATTGCA", 5), (1, 2, 3, 200, 201, 255, 3, 3))}
    got = ref.expected(counts, 5, 3, 200)
    assert got["graph"].S == {x for x, v in counts.items() if 3 <= v <= 200} and got["n_nodes"] == 4
    assert int(got["depth"].sum()) == 3 + 200 + 3 + 3


# ------------------------------------------------------------------ the inputs of the seam tests --
def _marked(text, *rows):
    return all(f"\n>{r}\n".encode("ascii") in text for r in rows)


def test_small_graph_inputs_hold_every_feature():
    """What test_gpu_unitig_seams.py relies on at k = 1 and k = 3, on the reference alone."""
    assert ui.canonical(1) == [0, 1] and len(ui.k1_tables()) == 9 and len(ui.canonical(3)) == 32
    for mn, mx in ui.K1_WINDOWS:
        rows = set()
        for counts in ui.k1_tables():
            want = ref.expected(counts, 1, mn, mx)
            ref.check_invariants(want)
            rows.add(len(want["n_kmers"]))
            assert want["n_nodes"] == want["n_branching"] == want["n_linear"] == len(want["n_kmers"]) and want["n_circular"] == 0
            assert want["n_kmers"].tolist() == [1] * want["n_nodes"] and len(want["fasta"]) == 5 * want["n_nodes"]      # every node branches
        assert rows == {0, 1, 2}, (mn, mx, rows)
    cases = ui.k3_cases()
    assert len(ui.k3_subsets()) == 1500 and len(cases) == 2000 and sum(c[2:4] == (2, 3) for c in cases) == 500
    found, linear, rings, empty = set(), set(), [], 0
    for name, counts, mn, mx, want in cases:
        assert all(1 <= v <= 3 for v in counts.values()) and set(counts) <= set(ui.canonical(3))
        empty += want["n_nodes"] == 0
        if (mn, mx) != (1, 255):
            continue
        found |= ui.features(want["graph"])
        linear |= set(want["n_kmers"][want["circular"] == 0].tolist())
        rings += want["n_kmers"][want["circular"] == 1].tolist()
    assert found == {"self_loop", "hairpin", "double_edge"}, found
    assert linear >= {1, 2, 3, 4, 5}, linear
    assert len(rings) >= 3 and set(rings) >= {2, 3}, rings
    assert empty >= 1                                        # a table without a node among them
    for name, counts, mn, mx, want in cases[::40]:
        ref.check_invariants(want)


def test_ring_inputs_hold_what_the_ring_tests_rely_on():
    """What sections B, C and E of test_gpu_unitig_seams.py rely on, on the reference alone."""
    counts = ui.ring_table()
    assert ui.RING_K == 11 and sum(v == ui.RING_COUNT for v in counts.values()) == 18174 and len(counts) == 19314
    rows = {}
    for mn, mx, M in ui.RING_BUILDS:
        want = ui.ring_expected(mn, mx, M)
        ref.check_invariants(want, M)
        rows[mn, mx, M] = (want["n_linear"], want["n_circular"], want["n_short"])
        assert want["n_branching"] == 0
    assert rows == {(1, 2, 1): (0, 1100, 0), (1, 255, 1): (95, 1100, 0), (1, 2, 12): (0, 1028, 72), (1, 255, 12): (51, 1028, 116), (5, 5, 1): (95, 0, 0)}, rows
    full, only = ui.ring_expected(1, 255, 1), ui.ring_expected(1, 2, 1)
    assert full["n_nodes"] == 19314 and len(full["fasta"]) == 38519 and only["n_nodes"] == 18174
    # row_base = 0: every decimal width begins inside the circular text; row_base = 95: the widths 3 and 4 do
    assert ui.linear_bytes(only) == 0 and _marked(b"\n" + only["fasta"], 0, 9, 10, 99, 100, 999, 1000)
    lin = ui.linear_bytes(full)
    assert 17 < lin < len(full["fasta"]) - 17 and _marked(full["fasta"][lin - 1:], 95, 99, 100, 999, 1000) and not _marked(full["fasta"][lin - 1:], 94)
    for M12, M1 in ((ui.ring_expected(1, 2, 12), only), (ui.ring_expected(1, 255, 12), full)):        # renumbered, not thinned out
        keep = M1["n_kmers"] >= 12
        assert np.array_equal(M12["first_addr"], M1["first_addr"][keep]) and M12["nodes_short"] == int(M1["n_kmers"][~keep].sum()) > 0
        assert ref.texts(M12) == [t for t, kept in zip(ref.texts(M1), keep) if kept]
    assert ui.linear_bytes(ui.ring_expected(5, 5, 1)) == len(ui.ring_expected(5, 5, 1)["fasta"]) == lin
    # the rebuild sequence: a window without a node, and an M above every unitig
    assert [b[:2] for b in ui.REBUILDS] == [(1, 255), (1, 2), (5, 5), (200, 255), (1, 255), (1, 255)]
    none, short = ui.ring_expected(*ui.REBUILDS[3]), ui.ring_expected(*ui.REBUILDS[5])
    assert none["n_nodes"] == 0 and len(none["n_kmers"]) == 0 and none["fasta"] == b""
    assert ui.REBUILDS[5][2] > full["longest_kmers"] and len(short["n_kmers"]) == 0 and short["fasta"] == b""
    assert short["nodes_short"] == short["n_nodes"] == 19314 and short["n_short"] == 1195 and short["longest_kmers"] == 0
    # One kept row per ring among all its nodes, spread over the rank workgroups (256 candidates each).  A ring's minimum is
    # the smallest of 11 to 22 random addresses, so the minima of these 1100 rings lie in the low third of their 71 groups
    # and cannot reach 50 of them; the 3000 rings of wide_ring_table() do.
    groups = ui.loop_candidate_groups(only)
    assert groups == ui.loop_candidate_groups(full) and 20 <= len(groups) < 50 and (only["n_nodes"] + 255) // 256 == 71
    wide = ui.wide_ring_expected(1)
    ref.check_invariants(wide)
    assert (wide["n_linear"], wide["n_circular"], wide["n_branching"]) == (0, ui.WIDE_RINGS, 0) and _marked(wide["fasta"], 999, 1000, 2999)
    assert len(ui.loop_candidate_groups(wide)) >= 50
    cut = ui.wide_ring_expected(12)
    assert 0 < cut["n_short"] == ui.WIDE_RINGS - cut["n_circular"] and len(ui.loop_candidate_groups(cut)) >= 50


def test_dense_input_needs_two_scan_rounds_and_six_digits():
    """More than 1024 rank workgroups of 256 ends each, and more than 100 000 rows; M = 3 keeps few of the candidates."""
    want = ui.dense_expected(1)
    ends = ui.ends_of(want)
    assert len(ends) > 262_144 + 256 and (len(ends) + 255) // 256 > 1024
    assert want["n_linear"] > 100_000 and _marked(want["fasta"], 99_999, 100_000) and want["n_branching"] > 0
    assert int(np.count_nonzero(ui.dense_table())) == want["n_nodes"] and want["graph"].S == set(np.flatnonzero(ui.dense_table()).tolist())
    kept = int((want["n_kmers"] >= 3).sum())                 # the rows of M = 3, without a second run of the reference
    assert 1000 < kept and 20 * kept < len(ends) and want["longest_kmers"] >= 3
    owners = set(want["first_addr"][want["n_kmers"] >= 3].tolist())
    kept_groups = {i // 256 for i, x in enumerate(sorted(ends)) if x in owners}
    assert max(kept_groups) >= 1024 and min(kept_groups) < 1024        # kept rows on both sides of the scan's seam


# ------------------------------------------------------------------ n50 ---------------------------
def test_n50():
    assert unitigs.n50([]) == 0 and unitigs.n50([7]) == 7
    assert unitigs.n50([2, 3, 4, 5, 6, 7, 8, 9, 10]) == 8                          # 54 bases: 10 + 9 + 8 = 27 >= 27
    assert unitigs.n50([1] * 10 + [10]) == 10 and unitigs.n50([1] * 11 + [10]) == 1
    assert unitigs.n50(np.array([5, 5, 5, 5], dtype=np.uint64)) == 5


# ------------------------------------------------------------------ the writers and the refusals --
FASTA = b">a\nACGGTCATTGCAGGCATTAGCAGCAGGAC\n>b\nGGTTTTTTTTTC\n>c\nACACACAC\n"
CALLS = []


def _stage(table, kmer_len, device, threads):
    return table.read_table_slice(0, 4 ** kmer_len), lambda: CALLS.append("freed")


def _run(ptr, kmer_len, mn, mx, M, device):
    want = ref.expected(ref.counts_of_table(ptr), kmer_len, mn, mx, M)
    out = {key: want[key] for key in ("first_addr", "n_kmers", "depth", "circular", "n_nodes", "n_branching", "n_linear", "n_circular", "n_short",
                                      "nodes_short", "longest_kmers")}
    return dict(out, bytes=len(want["fasta"]), links_s=0.5, paths_s=0.25, cycles_s=0.125, chunks=iter([want["fasta"][:10], want["fasta"][10:]]))


FAKES = dict(stage=_stage, run=_run, hbm_budget=1 << 40)


@pytest.fixture()
def project(tmp_path):
    return tmp_path, write_kin(tmp_path, "g.fa", FASTA, 5).path


def test_unitigs_writes_the_three_files(project):
    tmp_path, kin = project
    table = np.fromfile(kin, dtype=np.uint8)
    for n, (mn, mx, M) in enumerate(((1, 255, 1), (1, 1, 1), (1, 255, 3))):
        proj = str(tmp_path / f"run{n}")
        res = unitigs.unitigs_records(proj, [kin], min_count=mn, max_count=mx, min_kmers=M, **FAKES)
        want = ref.expected(ref.counts_of_table(table), 5, mn, mx, M)
        assert len(want["n_kmers"]) >= 2
        assert sorted(p.name for p in tmp_path.glob(f"run{n}.*")) == [f"run{n}.kmu", f"run{n}.kmu.json", f"run{n}.unitigs.fa"]       # no .tmp
        assert (tmp_path / f"run{n}.unitigs.fa").read_bytes() == want["fasta"]
        z = np.load(proj + ".kmu")
        assert sorted(z.files) == sorted(["first_addr", "n_kmers", "depth", "circular", "kmer_len", "min_count", "max_count", "min_kmers", "n_nodes"])
        assert z["first_addr"].dtype == z["n_kmers"].dtype == z["depth"].dtype == np.uint64 and z["circular"].dtype == np.uint8
        for key in ("first_addr", "n_kmers", "depth", "circular"):
            assert np.array_equal(z[key], want[key]), key
        assert (int(z["kmer_len"]), int(z["min_count"]), int(z["max_count"]), int(z["min_kmers"]), int(z["n_nodes"])) == (5, mn, mx, M, want["n_nodes"])
        meta = json.load(open(proj + ".kmu.json"))
        lengths = want["n_kmers"] + np.uint64(4)
        assert (meta["project_name"], meta["kmer_len"], meta["min_count"], meta["max_count"], meta["min_kmers"], meta["n_nodes"]) == \
            (proj, 5, mn, mx, M, want["n_nodes"])
        assert (meta["n_unitigs"], meta["n_circular"], meta["n_branching"], meta["n_short"], meta["nodes_short"]) == \
            (len(want["n_kmers"]), want["n_circular"], want["n_branching"], want["n_short"], want["nodes_short"])
        assert (meta["bases"], meta["longest"], meta["n50"], meta["output"]) == (int(lengths.sum()), int(lengths.max()), unitigs.n50(lengths), proj + ".unitigs.fa")
        assert (meta["links_s"], meta["paths_s"], meta["cycles_s"]) == (0.5, 0.25, 0.125)
        assert len(meta["data"]) == 1 and meta["data"][0]["pos"] == 0 and meta["data"][0]["header"]["kmer_len"] == 5
        assert res["n_unitigs"] == len(want["n_kmers"]) and res["output"] == proj + ".unitigs.fa"
    assert CALLS and set(CALLS) == {"freed"}
    got = unitigs.build_unitigs(kin, **FAKES)                 # without a file: the bytes come back
    want = ref.expected(ref.counts_of_table(table), 5)
    assert got["fasta"] == want["fasta"] and "output" not in got and got["n_circular"] == want["n_circular"] >= 1


def test_last_line_of_the_tool(project, capsys, monkeypatch):
    tmp_path, kin = project
    monkeypatch.setattr(unitigs, "stage_table", _stage)
    monkeypatch.setattr(unitigs, "run_build", _run)
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(1 << 40))
    proj = str(tmp_path / "cli")
    unitigs.main([proj, kin, "--min-kmers", "2"])
    want = ref.expected(ref.counts_of_table(np.fromfile(kin, dtype=np.uint8)), 5, min_kmers=2)
    lengths = want["n_kmers"] + np.uint64(4)
    last = capsys.readouterr().out.strip().split("\n")[-1]
    assert last == f"{len(lengths)} unitigs ({want['n_circular']} circular) from {want['n_nodes']} k-mers, longest {int(lengths.max())} bases, " \
                   f"N50 {unitigs.n50(lengths)}, {proj}.unitigs.fa"


def test_refusals_come_before_any_file(project, capsys):
    tmp_path, kin = project
    bad = str(tmp_path / "bad")
    other = write_kin(tmp_path, "h.fa", FASTA, 5).path
    with pytest.raises(ValueError, match=r"exactly one table.*extract\.py .*--table"):
        unitigs.unitigs_records(bad, [kin, other], **FAKES)
    with pytest.raises(ValueError, match="exactly one table"):
        unitigs.unitigs_records(bad, [], **FAKES)
    for kw, msg in ((dict(min_count=0), "count window"), (dict(max_count=256), "count window"), (dict(min_count=9, max_count=3), "count window"),
                    (dict(min_kmers=0), "--min-kmers"), (dict(min_kmers=-3), "--min-kmers"), (dict(min_kmers=2.5), "--min-kmers"),
                    (dict(min_kmers=True), "--min-kmers")):
        with pytest.raises(ValueError, match=msg):
            unitigs.unitigs_records(bad, [kin], **kw, **FAKES)
    with pytest.raises(ValueError, match="does not exist"):
        unitigs.unitigs_records(bad, [tmp_path / "missing.05.kin"], **FAKES)
    with pytest.raises(ValueError, match="kin"):
        unitigs.unitigs_records(bad, [tmp_path / "g.fa"], **FAKES)
    with pytest.raises(ValueError, match=r"window 200-255"):                       # an empty window names the window and leaves no file
        unitigs.unitigs_records(bad, [kin], min_count=200, **FAKES)
    assert not list(tmp_path.glob("bad*"))
    with pytest.raises(ValueError, match="HBM budget"):                            # the table and the link array: 2 * 4^5 bytes
        unitigs.unitigs_records(bad, [kin], stage=_stage, run=_run, hbm_budget=2 * 4 ** 5 - 1)
    for existing in ("bad.unitigs.fa", "bad.kmu", "bad.kmu.json"):
        (tmp_path / existing).write_bytes(b"mine")
        with pytest.raises(ValueError, match="already exists"):
            unitigs.unitigs_records(bad, [kin], **FAKES)
        assert (tmp_path / existing).read_bytes() == b"mine"
        (tmp_path / existing).unlink()
    assert not list(tmp_path.glob("bad*"))
    for k, msg in ((19, "beyond the unitigs path"), (4, "odd")):                   # tables that are no odd k <= 17
        stub = type("T", (), {"kmer_len": k, "index_file": f"t{k}.kin", "data_size": 4 ** k})()
        with pytest.raises(ValueError, match=msg):
            unitigs.build_unitigs(stub, **FAKES)
    for argv in ([bad, kin, other], [bad, kin, "--min-count", "0"], [bad, kin, "--min-kmers", "0"]):      # the command line
        with pytest.raises(SystemExit) as exc:
            unitigs.main(argv)
        err = capsys.readouterr().err
        assert exc.value.code == 1 and err.startswith("error: ") and (len(argv) != 3 or "extract.py" in err)
    assert not list(tmp_path.glob("bad*"))
    assert [str(p) for p in unitigs.kmu_paths("p")] == ["p.unitigs.fa", "p.kmu", "p.kmu.json"]


# ------------------------------------------------------------------ C-ABI surface ---------------
def test_unitig_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "pykmer_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines()}
    lib = _lib.load()
    for name in UNITIG_SYMBOLS:
        assert name in declared and name in exported and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.pk_version() == 3 and "typedef struct pk_unitig pk_unitig;" in text
    for words in ("COMPACTABLE EDGE", "canon(o) != canon(t)", "smaller canonical address"):      # the definition stands in the header
        assert words in header
    assert os.path.exists(os.path.join(ROOT, "unitigs.py")) and os.path.exists(os.path.join(ROOT, "pykmer_amd", "csrc", "kmer_unitig.hip"))
    assert len(_lib.UNITIG_TOTALS) == 8


def test_arguments_are_checked_without_a_device():
    lib = _lib.load()
    h = ctypes.c_void_p()
    for k in (0, 2, 16, 19, -1):
        assert lib.pk_unitig_create(ctypes.byref(h), k, 0) == _lib.PK_ERR_ARG
        with pytest.raises(ValueError):
            _lib.Unitigs(k)
    assert lib.pk_unitig_create(None, 5, 0) == _lib.PK_ERR_ARG and lib.pk_unitig_create(ctypes.byref(h), 5, 64) == _lib.PK_ERR_ARG
    buf = np.zeros(8, dtype=np.uint64)
    assert lib.pk_unitig_build(None, None, 1, 255, 1, buf.ctypes.data) == _lib.PK_ERR_ARG
    assert lib.pk_unitig_rows(None, None, None, None, None, 0) == _lib.PK_ERR_ARG
    assert lib.pk_unitig_text(None, None, 0, 0) == _lib.PK_ERR_ARG and lib.pk_unitig_timings(None, None) == _lib.PK_ERR_ARG
    with _lib.Unitigs(17) as u:                              # creating one touches no device; nothing is built yet
        assert lib.pk_unitig_rows(u._h, None, None, None, None, 0) == _lib.PK_ERR_STATE
        assert lib.pk_unitig_text(u._h, None, 0, 0) == _lib.PK_ERR_STATE
        assert u.timings() == {"links_s": 0.0, "paths_s": 0.0, "cycles_s": 0.0, "builds": 0}
        for args in ((None, 1, 255, 1), (ctypes.c_void_p(8), 1, 255, 1), (ctypes.c_void_p(64), 0, 255, 1), (ctypes.c_void_p(64), 3, 2, 1),
                     (ctypes.c_void_p(64), 1, 256, 1), (ctypes.c_void_p(64), 1, 255, 0)):
            assert lib.pk_unitig_build(u._h, *args, buf.ctypes.data) == _lib.PK_ERR_ARG, args
    lib.pk_unitig_destroy(None)
