"""The unitig graph without a GPU: the reference module of the edges against hand-written cases and its own invariants, the
writers of unitigs.py --gfa through the stage / run hooks, the refusals, and the C-ABI surface."""
import ctypes
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import unitig_graph_ref as gref
import unitig_inputs as ui
import unitig_ref as ref
from host_support import ROOT, write_kin
from pykmer_amd import _lib, unitigs

GRAPH_SYMBOLS = ("pk_unitig_graph", "pk_unitig_edges", "pk_unitig_gfa_text", "pk_unitig_graph_timings")


def _of(counts, k, M=1, **kw):
    want = ref.expected(counts, k, min_kmers=M, **kw)
    got = gref.graph(want)
    gref.check_invariants(want, got, M)
    return want, got


def _named(got):
    return [f"{r}{'+-'[s]}>{q}{'+-'[u]}" for r, s, q, u, _ in got["edges"]]


# ------------------------------------------------------------------ the reference: hand cases -----
def test_worked_examples():
    want, got = _of(ui.counts_of(["AAAAATTTTT"], 5), 5)
    assert ref.texts(want) == ["AAAAA", "AAAATT"]
    assert _named(got) == ["0+>0+", "0+>1+", "0->0-", "1+>1-", "1->0-"]
    assert got["edge_from"].tolist() == [0, 0, 0, 1, 1] and got["edge_to"].tolist() == [0, 1, 0, 1, 0] and got["edge_orient"].tolist() == [0, 0, 3, 2, 3]
    assert (got["n_edges"], got["edges_dropped"], got["n_dead_ends"]) == (5, 0, 0)
    assert got["gfa"] == (b"H\tVN:Z:1.0\nS\t0\tAAAAA\tLN:i:5\tKC:i:1\nS\t1\tAAAATT\tLN:i:6\tKC:i:2\n"
                          b"L\t0\t+\t0\t+\t4M\nL\t0\t+\t1\t+\t4M\nL\t0\t-\t0\t-\t4M\nL\t1\t+\t1\t-\t4M\nL\t1\t-\t0\t-\t4M\n")
    want, got = _of(ui.counts_of(["ACACACAC"], 5), 5)
    assert want["circular"].tolist() == [1] and _named(got) == ["0+>0+", "0->0-"] and got["n_dead_ends"] == 0
    assert got["gfa"] == b"H\tVN:Z:1.0\nS\t0\tACACAC\tLN:i:6\tKC:i:2\nL\t0\t+\t0\t+\t4M\nL\t0\t-\t0\t-\t4M\n"


def test_snp_bubble_and_y_branch():
    k = 9
    rng, seen = random.Random(9), set()
    left, right = ui.distinct_sequence(rng, 20, k, seen), ui.distinct_sequence(rng, 20, k, seen)
    want, got = _of(ui.counts_of([left + "A" + right, left + "C" + right], k), k)
    sizes = want["n_kmers"].tolist()
    assert sorted(sizes) == [9, 9, 12, 12] and got["n_edges"] == 8
    alleles, flanks = {r for r in range(4) if sizes[r] == 9}, {r for r in range(4) if sizes[r] == 12}
    joined = {frozenset((r, q)) for r, _, q, _, _ in got["edges"]}
    assert joined == {frozenset((a, f)) for a in alleles for f in flanks}          # both alleles link to both flanks, nothing else
    assert got["n_dead_ends"] == 2                                                   # the outer end of each flank
    stem, arm1, arm2 = (ui.distinct_sequence(rng, 25, k, seen) for _ in range(3))
    want, got = _of(ui.counts_of([stem + arm1, stem[-(k - 1):] + arm2], k), k)
    assert want["n_branching"] == 1 and len(want["n_kmers"]) == 3 and got["n_edges"] == 4 and got["n_dead_ends"] == 3
    fork = [r for r, s in {e[:2] for e in got["edges"]} if sum(1 for e in got["edges"] if e[:2] == (r, s)) == 2]
    assert len(fork) == 1                                                            # the stem's end forks into the two arms


@pytest.mark.parametrize("k", [3, 5, 7])
def test_invariants_on_random_sets(k):
    if k == 3:
        for counts in ui.k3_subsets()[:600]:
            _of(counts, 3)
        return
    rng = random.Random(70 + k)
    for d in (0.02, 0.1, 0.3, 0.6, 1.0):
        counts = {x: 1 + x % 9 for x in range(4 ** k) if x == ref.canon(x, k) and (d == 1.0 or rng.random() < d)}
        want, got = _of(counts, k)
        if d == 1.0:                                         # every row is one node with 4 successors on either side
            assert want["n_kmers"].tolist() == [1] * (4 ** k // 2) and got["n_edges"] == 4 ** (k + 1) and got["n_dead_ends"] == 0
            selfs = sum(1 for r, s, q, u, _ in got["edges"] if r == q and s != u)
            assert k != 5 or (got["n_edges"], selfs) == (4096, 64)


def min_kmers_table() -> dict:
    """k = 7, a tenth of the canonical addresses: mostly single nodes, and unitigs of 2, 3 and more k-mers between them."""
    rng = random.Random(75)
    return {x: 1 for x in range(4 ** 7) if x == ref.canon(x, 7) and rng.random() < 0.1}


def test_min_kmers_drops_edges():
    """M = 2 and 3: edges into dropped unitigs are counted, not written, and the rows are numbered anew.  The precondition of
    the GPU test of --min-kmers."""
    counts, k = min_kmers_table(), 7
    full_want, full = _of(counts, k)
    seen = 0
    for M in (2, 3):
        want, got = _of(counts, k, M)
        assert got["edges_dropped"] > 0 and 0 < got["n_edges"] < full["n_edges"]
        keep = np.flatnonzero(full_want["n_kmers"] >= M)
        assert not np.array_equal(keep, np.arange(keep.size))                        # a row index changes
        old = {int(r): i for i, r in enumerate(keep)}
        assert [e[:4] for e in got["edges"]] == [(old[r], s, old[q], u) for r, s, q, u, _ in full["edges"] if r in old and q in old]
        seen += 1
    assert seen == 2
    want, got = _of(counts, k, 1000)
    assert len(want["n_kmers"]) == 0 and got["gfa"] == gref.HEADER and got["n_edges"] == got["n_dead_ends"] == got["edges_dropped"] == 0


def test_parse_gfa_reads_back_what_the_reference_writes():
    want, got = _of(ui.counts_of(["AAAAATTTTT"], 5), 5)
    parsed = gref.parse_gfa(got["gfa"])
    assert parsed["segments"] == [("0", "AAAAA", 5, 1), ("1", "AAAATT", 6, 2)]
    assert parsed["links"] == [(0, 0, 0, 0, 4), (0, 0, 1, 0, 4), (0, 1, 0, 1, 4), (1, 0, 1, 1, 4), (1, 1, 0, 1, 4)]
    assert gref.parse_gfa(gref.HEADER) == {"segments": [], "links": []}
    broken = dict(parsed, links=[(0, 0, 1, 1, 4)])                                   # AAAAA does not run into rc(AAAATT)
    with pytest.raises(AssertionError):
        gref.check_overlaps(broken, want["graph"])


# ------------------------------------------------------------------ the writers and the refusals --
FASTA = b">a\nACGGTCATTGCAGGCATTAGCAGCAGGAC\n>b\nGGTTTTTTTTTC\n>c\nACACACAC\n"
BASE_KEYS = ["first_addr", "n_kmers", "depth", "circular", "kmer_len", "min_count", "max_count", "min_kmers", "n_nodes"]
CALLS = []


def _stage(table, kmer_len, device, threads):
    return table.read_table_slice(0, 4 ** kmer_len), lambda: None


def _run(ptr, kmer_len, mn, mx, M, device, **kw):
    CALLS.append(kw)
    want = ref.expected(ref.counts_of_table(ptr), kmer_len, mn, mx, M)
    out = {key: want[key] for key in ("first_addr", "n_kmers", "depth", "circular", "n_nodes", "n_branching", "n_linear", "n_circular", "n_short",
                                      "nodes_short", "longest_kmers")}
    out.update(bytes=len(want["fasta"]), links_s=0.5, paths_s=0.25, cycles_s=0.125, chunks=iter([want["fasta"][:10], want["fasta"][10:]]))
    if kw:
        assert kw == {"gfa": True}
        g = gref.graph(want)
        out.update({key: g[key] for key in ("edge_from", "edge_to", "edge_orient", "n_edges", "edges_dropped", "n_dead_ends")})
        out.update(edges_s=0.0625, gfa_s=0.03125, gfa_chunks=iter([g["gfa"][:7], g["gfa"][7:]]))
    return out


FAKES = dict(stage=_stage, run=_run, hbm_budget=1 << 40)


@pytest.fixture()
def project(tmp_path):
    return tmp_path, write_kin(tmp_path, "g.fa", FASTA, 5).path


def test_gfa_writes_the_four_files(project):
    tmp_path, kin = project
    table = np.fromfile(kin, dtype=np.uint8)
    for n, (mn, mx, M) in enumerate(((1, 255, 1), (1, 255, 2))):
        proj = str(tmp_path / f"run{n}")
        del CALLS[:]
        res = unitigs.unitigs_records(proj, [kin], min_count=mn, max_count=mx, min_kmers=M, gfa=True, **FAKES)
        assert CALLS == [{"gfa": True}]
        want = ref.expected(ref.counts_of_table(table), 5, mn, mx, M)
        g = gref.graph(want)
        assert g["n_edges"] >= 2 and (M == 1 or g["edges_dropped"] > 0)
        assert sorted(p.name for p in tmp_path.glob(f"run{n}.*")) == [f"run{n}.kmu", f"run{n}.kmu.json", f"run{n}.unitigs.fa", f"run{n}.unitigs.gfa"]
        assert (tmp_path / f"run{n}.unitigs.fa").read_bytes() == want["fasta"] and (tmp_path / f"run{n}.unitigs.gfa").read_bytes() == g["gfa"]
        z = np.load(proj + ".kmu")
        assert sorted(z.files) == sorted(BASE_KEYS + ["edge_from", "edge_to", "edge_orient"])
        assert z["edge_from"].dtype == z["edge_to"].dtype == np.uint64 and z["edge_orient"].dtype == np.uint8
        for key in ("edge_from", "edge_to", "edge_orient", "first_addr", "n_kmers"):
            assert np.array_equal(z[key], g[key] if key in g else want[key]), key
        meta = json.load(open(proj + ".kmu.json"))
        assert (meta["gfa"], meta["n_edges"], meta["edges_dropped"], meta["n_dead_ends"], meta["edges_s"], meta["gfa_s"]) == \
            (proj + ".unitigs.gfa", g["n_edges"], g["edges_dropped"], g["n_dead_ends"], 0.0625, 0.03125)
        assert meta["output"] == proj + ".unitigs.fa" and meta["n_unitigs"] == len(want["n_kmers"])
        assert res["gfa_output"] == proj + ".unitigs.gfa" and res["n_edges"] == g["n_edges"] and "gfa" not in res
    # without gfa: the run hook gets the six positional arguments of before, and no key or file of the graph appears
    del CALLS[:]
    res = unitigs.unitigs_records(str(tmp_path / "plain"), [kin], **FAKES)
    assert CALLS == [{}] and not [key for key in res if "edge" in key or "gfa" in key]
    assert sorted(p.name for p in tmp_path.glob("plain.*")) == ["plain.kmu", "plain.kmu.json", "plain.unitigs.fa"]
    assert sorted(np.load(str(tmp_path / "plain.kmu")).files) == sorted(BASE_KEYS)
    meta = json.load(open(tmp_path / "plain.kmu.json"))
    assert not [key for key in meta if "edge" in key or "gfa" in key or key == "n_dead_ends"]
    # without files: the bytes come back
    got = unitigs.build_unitigs(kin, gfa=True, **FAKES)
    g = gref.graph(ref.expected(ref.counts_of_table(table), 5))
    assert got["gfa"] == g["gfa"] and "gfa_output" not in got and np.array_equal(got["edge_orient"], g["edge_orient"])
    assert (got["n_edges"], got["edges_dropped"], got["n_dead_ends"], got["edges_s"], got["gfa_s"]) == (g["n_edges"], 0, g["n_dead_ends"], 0.0625, 0.03125)


def test_last_line_of_the_tool(project, capsys, monkeypatch):
    tmp_path, kin = project
    monkeypatch.setattr(unitigs, "stage_table", _stage)
    monkeypatch.setattr(unitigs, "run_build", _run)
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(1 << 40))
    want = ref.expected(ref.counts_of_table(np.fromfile(kin, dtype=np.uint8)), 5, min_kmers=2)
    lengths = want["n_kmers"] + np.uint64(4)
    plain = f"{len(lengths)} unitigs ({want['n_circular']} circular) from {want['n_nodes']} k-mers, longest {int(lengths.max())} bases, " \
            f"N50 {unitigs.n50(lengths)}, "
    proj = str(tmp_path / "cli")
    unitigs.main([proj, kin, "--min-kmers", "2", "--gfa"])
    last = capsys.readouterr().out.strip().split("\n")[-1]
    assert last == plain + f"{proj}.unitigs.fa, {gref.graph(want)['n_edges']} edges in {proj}.unitigs.gfa"
    unitigs.main([proj + "2", kin, "--min-kmers", "2"])
    assert capsys.readouterr().out.strip().split("\n")[-1] == plain + f"{proj}2.unitigs.fa"


def test_refusals_come_before_any_file(project):
    tmp_path, kin = project
    bad = str(tmp_path / "bad")
    (tmp_path / "bad.unitigs.gfa").write_bytes(b"mine")
    with pytest.raises(ValueError, match="already exists"):
        unitigs.unitigs_records(bad, [kin], gfa=True, **FAKES)
    assert [p.name for p in tmp_path.glob("bad*")] == ["bad.unitigs.gfa"] and (tmp_path / "bad.unitigs.gfa").read_bytes() == b"mine"
    unitigs.unitigs_records(bad, [kin], **FAKES)             # without --gfa that file is nobody's business
    assert (tmp_path / "bad.unitigs.gfa").read_bytes() == b"mine"
    with pytest.raises(ValueError, match=r"window 200-255"):
        unitigs.unitigs_records(str(tmp_path / "none"), [kin], min_count=200, gfa=True, **FAKES)
    assert not list(tmp_path.glob("none*"))
    assert [str(p) for p in unitigs.kmu_paths("p")] == ["p.unitigs.fa", "p.kmu", "p.kmu.json"] and str(unitigs.gfa_path("p")) == "p.unitigs.gfa"


# ------------------------------------------------------------------ C-ABI surface ---------------
def test_graph_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "pykmer_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines()}
    lib = _lib.load()
    for name in GRAPH_SYMBOLS:
        assert name in declared and name in exported and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.pk_version() == 3 and len(_lib.UNITIG_TOTALS) == 8 and len(_lib.UNITIG_GRAPH_TOTALS) == 4
    for words in ("ORIENTED ROW", "tail(r,-) = rc(o_n)", "MIRROR", "COUNT IDENTITY"):      # the definition stands in the header
        assert words in header


def test_arguments_are_checked_without_a_device():
    lib = _lib.load()
    buf = np.zeros(4, dtype=np.uint64)
    assert lib.pk_unitig_graph(None, buf.ctypes.data) == _lib.PK_ERR_ARG
    assert lib.pk_unitig_edges(None, None, None, None, 0) == _lib.PK_ERR_ARG
    assert lib.pk_unitig_gfa_text(None, None, 0, 0) == _lib.PK_ERR_ARG and lib.pk_unitig_graph_timings(None, None) == _lib.PK_ERR_ARG
    with _lib.Unitigs(17) as u:                              # creating one touches no device; nothing is built yet
        assert lib.pk_unitig_graph(u._h, None) == _lib.PK_ERR_ARG and lib.pk_unitig_graph_timings(u._h, None) == _lib.PK_ERR_ARG
        assert lib.pk_unitig_graph(u._h, buf.ctypes.data) == _lib.PK_ERR_STATE
        assert lib.pk_unitig_edges(u._h, None, None, None, 0) == _lib.PK_ERR_STATE
        assert lib.pk_unitig_gfa_text(u._h, None, 0, 0) == _lib.PK_ERR_STATE
        for call in (u.graph, u.edges, u.gfa_text):           # the wrapper lets the library decide
            with pytest.raises(_lib.PkError) as exc:
                call()
            assert exc.value.code == _lib.PK_ERR_STATE
        assert u.graph_timings() == {"edges_s": 0.0, "gfa_s": 0.0}
        assert u.timings() == {"links_s": 0.0, "paths_s": 0.0, "cycles_s": 0.0, "builds": 0}
