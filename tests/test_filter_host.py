"""CPU: the filter path's rule, its pair rules, its refusals, its file names and files, and the selector's C-ABI surface.
No call here touches a GPU: the lookup is stood in for by query_ref, the selection by filter_ref."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import filter_ref
import query_ref
from fastq_qual_ref import mask_fastq_to_fasta
from host_support import stage_host, write_kin
from pykmer_amd import _lib, filter as kfilter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECT_SYMBOLS = ("pk_select_create", "pk_select_set_records", "pk_select_feed", "pk_select_feed_device", "pk_select_finish",
                  "pk_select_timings", "pk_select_destroy")


# ------------------------------------------------------------------ the rule --------------------
def _both(hits, n_valid, H=1, P=0, M=1):
    keep, match = kfilter.decide(np.array(hits, dtype=np.uint64).reshape(len(n_valid), -1), np.array(n_valid, dtype=np.uint64), H, P, M)
    want_keep, want_match = filter_ref.decide(np.array(hits).reshape(len(n_valid), -1), n_valid, H, P, M)
    assert keep.dtype == match.dtype == np.uint8
    assert keep.tolist() == [int(v) for v in want_keep] and match.tolist() == [[int(v) for v in row] for row in want_match]
    return keep.tolist(), match.tolist()


def test_decide_edges_of_h_p_and_m():
    hits, n_valid = [[0, 5, 9], [4, 5, 6], [10, 0, 0], [0, 0, 0]], [10, 10, 10, 10]
    assert _both(hits, n_valid)[0] == [1, 1, 1, 0]                         # H = 1: a single hit matches
    assert _both(hits, n_valid, H=5)[1] == [[0, 1, 1], [0, 1, 1], [1, 0, 0], [0, 0, 0]]   # hits == H matches, H - 1 does not
    assert _both(hits, n_valid, H=5, M=2)[0] == [1, 1, 0, 0]
    assert _both(hits, n_valid, H=5, M=3)[0] == [0, 0, 0, 0]
    assert _both(hits, n_valid, M=3)[0] == [0, 1, 0, 0]                    # M = N: every table
    assert _both(hits, n_valid, P=50)[1] == [[0, 1, 1], [0, 1, 1], [1, 0, 0], [0, 0, 0]]   # 5 of 10 is 50 %
    assert _both(hits, n_valid, P=51)[1] == [[0, 0, 1], [0, 0, 1], [1, 0, 0], [0, 0, 0]]
    assert _both(hits, n_valid, P=100)[1] == [[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0]]  # P = 100: every window hits
    assert _both(hits, n_valid, H=10, P=100)[0] == [0, 0, 1, 0]


def test_decide_without_a_valid_window_never_matches():
    assert _both([[0], [0]], [0, 1], P=0) == ([0, 0], [[0], [0]])
    # hits cannot exceed n_valid in a real result; the rule itself must still refuse a record without windows
    assert _both([[3]], [0], H=1, P=0)[0] == [0]


def test_decide_is_exact_where_the_products_meet():
    """100 * hits == P * n_valid matches and one hit fewer does not, also where float arithmetic would round: 3 * 33 < 100
    and at sizes beyond 2^53."""
    assert _both([[33], [34]], [100, 100], P=34)[0] == [0, 1]
    assert _both([[1], [1]], [3, 4], P=33)[0] == [1, 0]                    # 100 >= 99, but 100 < 132
    v = 2 ** 53 + 1                                                        # no double holds it
    assert _both([[v], [v - 1]], [v, v], P=100)[0] == [1, 0]
    n = 2 ** 60
    assert _both([[n // 4], [n // 4 - 1]], [n, n], P=25)[0] == [1, 0]      # 100 * hits is beyond 64 bits
    rng = np.random.default_rng(7)
    n_valid = rng.integers(0, 50, 200)
    hits = np.minimum(rng.integers(0, 50, (200, 4)), n_valid[:, None])
    for H, P, M in ((1, 0, 1), (2, 10, 2), (1, 33, 1), (3, 67, 4), (1, 100, 1)):
        _both(hits, n_valid, H, P, M)


def test_pair_rules():
    a, b = np.array([1, 1, 0, 0], dtype=np.uint8), np.array([1, 0, 1, 0], dtype=np.uint8)
    assert kfilter.pair_flags(a, b).tolist() == [1, 1, 1, 0] == kfilter.pair_flags(a, b, "any").tolist()
    assert kfilter.pair_flags(a, b, "both").tolist() == [1, 0, 0, 0]
    with pytest.raises(ValueError, match="same number of records"):
        kfilter.pair_flags(a, b[:3])
    with pytest.raises(ValueError, match="pair-rule"):
        kfilter.pair_flags(a, b, "either")


# ------------------------------------------------------------------ a run without a device ------
FASTA = (b"junk before the first header\n>  spaced name\nACGTTGCAAGGTCA\nGGTACC\n>none\nNNNN\n>short\nAC\n"
         b">third rec\nTTGACCAGGTAACGTACGTTAGC\nACGT\n>last\nGATTACAGATTACA")


def _fastq(n=6, seed=3, crlf=False):
    rng = np.random.default_rng(seed)
    nl = b"\r\n" if crlf else b"\n"
    recs = []
    for i in range(n):
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 20 + 3 * i)].tobytes()
        qual = bytes(rng.integers(35, 74, len(seq)).astype(np.uint8))
        recs.append(b"@read%d/x" % i + nl + seq + nl + b"+" + nl + (b"@" + qual[1:] if i % 2 else qual) + nl)
    return b"".join(recs)


def _run(query_file, kmer_len, ptrs, mn, mx, device, first, min_qual_byte=0):
    text = open(query_file, "rb").read()
    fmt = "fastq" if query_file.endswith(".fq") else "fasta"
    if fmt == "fastq" and min_qual_byte:
        want = query_ref.expected(mask_fastq_to_fasta(text, min_qual_byte)[0], kmer_len, ptrs, mn, mx)
    else:
        want = query_ref.expected(text, kmer_len, ptrs, mn, mx, fmt)
    starts = filter_ref.record_starts_ref(text, fmt)
    out = {key: want[key] for key in ("seq_len", "n_valid", "hits", "depth")}
    out.update(name_off=starts[:-1] + np.uint64(1), n_bytes=len(text), names=[f"r{i}" for i in range(len(starts) - 1)])
    return out


def _select(input_file, keep, out_file, starts=None, device=0):
    text = open(input_file, "rb").read()
    assert starts is not None and len(starts) == len(keep) + 1
    kept = filter_ref.select_bytes(text, starts, keep)
    with kfilter.atomic_write(out_file, "wb") as fh:
        fh.write(kept)
    return {"n_records": len(keep), "n_kept": int(np.count_nonzero(keep)), "bytes_in": len(text), "bytes_kept": len(kept)}


FAKES = dict(run=_run, stage=stage_host, select=_select, hbm_budget=1 << 40)


@pytest.fixture()
def project(tmp_path):
    k = 5
    kins = [write_kin(tmp_path, "donor.fa", b">d\nTTGACCAGGTAACGTACGTTAGCACGT\n", k).path, write_kin(tmp_path, "other.fa", b">o\nGATTACAGATTACAGGTACC\n", k).path]
    q = tmp_path / "reads.fa"
    q.write_bytes(FASTA)
    return tmp_path, kins, str(q)


def test_filter_writes_the_matching_records_and_the_decision(project):
    tmp_path, kins, q = project
    proj = str(tmp_path / "run")
    res = kfilter.filter(proj, q, kins[:1], min_percent=50, **FAKES)
    starts = filter_ref.record_starts_ref(FASTA)
    want = query_ref.expected(FASTA, 5, [np.fromfile(kins[0], dtype=np.uint8)], 1, 255)
    keep = np.array(filter_ref.decide(want["hits"], want["n_valid"], 1, 50, 1)[0], dtype=np.uint8)
    assert keep.tolist() == [0, 0, 0, 1, 0] and np.array_equal(res["keep"], keep) and np.array_equal(res["starts"], starts)
    assert sorted(p.name for p in tmp_path.glob("run.*")) == ["run.kept.fa", "run.kmf", "run.kmf.json"]      # no .tmp, no rest
    assert (tmp_path / "run.kept.fa").read_bytes() == b">third rec\nTTGACCAGGTAACGTACGTTAGC\nACGT\n"
    z = np.load(proj + ".kmf")
    assert sorted(z.files) == sorted(["keep", "match", "hits", "n_valid", "seq_len", "kmer_len", "min_count", "max_count", "min_hits", "min_percent",
                                      "min_tables", "invert", "pair_rule"])
    assert z["keep"].dtype == z["match"].dtype == np.uint8 and z["hits"].dtype == z["n_valid"].dtype == z["seq_len"].dtype == np.uint64
    assert z["keep"].shape == (5,) and z["match"].shape == z["hits"].shape == (5, 1)
    assert np.array_equal(z["keep"], keep) and np.array_equal(z["hits"], want["hits"]) and np.array_equal(z["n_valid"], want["n_valid"])
    assert (int(z["min_hits"]), int(z["min_percent"]), int(z["min_tables"]), bool(z["invert"])) == (1, 50, 1, False)
    meta = json.load(open(proj + ".kmf.json"))
    for key in ("project_name", "kmer_len", "min_count", "max_count", "query_file", "data"):                 # the .kmq.json's, without records
        assert key in meta
    assert "records" not in meta and "min_qual" not in meta
    assert (meta["min_hits"], meta["min_percent"], meta["min_tables"], meta["invert"], meta["pair_rule"]) == (1, 50, 1, False, None)
    assert meta["n_records"] == 5 and meta["n_kept"] == 1 and meta["outputs"] == [proj + ".kept.fa"]
    assert meta["files"] == [{"role": "kept", "file": proj + ".kept.fa", "input": q, "n_records": 5, "n_kept": 1, "bytes_in": len(FASTA),
                              "bytes_kept": len(b">third rec\nTTGACCAGGTAACGTACGTTAGC\nACGT\n")}]


def test_invert_and_rest_split_the_records(project):
    tmp_path, kins, q = project
    proj = str(tmp_path / "inv")
    tables = [np.fromfile(kin, dtype=np.uint8) for kin in kins]
    want = query_ref.expected(FASTA, 5, tables, 1, 255)
    starts = filter_ref.record_starts_ref(FASTA)
    matched = np.array(filter_ref.decide(want["hits"], want["n_valid"], 2, 0, 1)[0])
    assert matched.any() and not matched.all() and not matched[1] and not matched[2]    # no window, no match
    res = kfilter.filter(proj, q, kins, min_hits=2, invert=True, rest=True, **FAKES)
    assert res["keep"].tolist() == (~matched).astype(int).tolist()
    kept, rest = (tmp_path / "inv.kept.fa").read_bytes(), (tmp_path / "inv.rest.fa").read_bytes()
    assert kept == filter_ref.select_bytes(FASTA, starts, ~matched) and rest == filter_ref.select_bytes(FASTA, starts, matched)
    assert b">none\nNNNN\n>short\nAC\n" in kept and b"junk" not in kept + rest
    assert len(kept) + len(rest) == len(FASTA) - len(b"junk before the first header\n")
    assert (kept if not matched[4] else rest).endswith(b">last\nGATTACAGATTACA")            # the missing final newline stays missing
    assert sorted(p.name for p in tmp_path.glob("inv.*")) == ["inv.kept.fa", "inv.kmf", "inv.kmf.json", "inv.rest.fa"]
    both = kfilter.filter(str(tmp_path / "m2"), q, kins, min_tables=2, min_percent=100, **FAKES)
    want2 = np.array(filter_ref.decide(want["hits"], want["n_valid"], 1, 100, 2)[0])
    assert both["keep"].tolist() == want2.astype(int).tolist() and not want2.any() and (tmp_path / "m2.kept.fa").read_bytes() == b""


def test_mates_share_their_flags(project):
    tmp_path, kins, _ = project
    fq1, fq2 = _fastq(6, seed=3), _fastq(6, seed=4, crlf=True)
    (tmp_path / "r_1.fq").write_bytes(fq1)
    (tmp_path / "r_2.fq").write_bytes(fq2)
    table = write_kin(tmp_path, "bait.fa", b">b\n" + fq1.split(b"\n")[1] + b"\n" + fq2.split(b"\r\n")[9] + b"\n", 7).path
    t = np.fromfile(table, dtype=np.uint8)
    m1 = np.array(filter_ref.decide(*[query_ref.expected(fq1, 7, [t], 1, 255, "fastq")[key] for key in ("hits", "n_valid")])[0])
    m2 = np.array(filter_ref.decide(*[query_ref.expected(fq2, 7, [t], 1, 255, "fastq")[key] for key in ("hits", "n_valid")])[0])
    assert m1[0] and m2[2] and (m1 | m2).sum() > (m1 & m2).sum()             # the two rules differ
    for rule, flags in (("any", m1 | m2), ("both", m1 & m2), (None, m1 | m2)):
        proj = str(tmp_path / f"pair_{rule}")
        res = kfilter.filter(proj, str(tmp_path / "r_1.fq"), [table], mate=str(tmp_path / "r_2.fq"), pair_rule=rule, rest=True, **FAKES)
        assert res["keep"].tolist() == flags.astype(int).tolist()
        names = sorted(p.name for p in tmp_path.glob(f"pair_{rule}.*"))
        assert names == [f"pair_{rule}.{x}" for x in ("kept_1.fq", "kept_2.fq", "kmf", "kmf.json", "rest_1.fq", "rest_2.fq")]
        for n, fq in (("1", fq1), ("2", fq2)):
            starts = filter_ref.record_starts_ref(fq, "fastq")
            assert (tmp_path / f"pair_{rule}.kept_{n}.fq").read_bytes() == filter_ref.select_bytes(fq, starts, flags)
            assert (tmp_path / f"pair_{rule}.rest_{n}.fq").read_bytes() == filter_ref.select_bytes(fq, starts, ~flags)
        z = np.load(proj + ".kmf")
        assert {"hits_2", "n_valid_2", "match_2"} <= set(z.files) and z["match_2"][:, 0].tolist() == m2.astype(int).tolist()
        assert json.load(open(proj + ".kmf.json"))["pair_rule"] == (rule or "any")


def test_min_qual_changes_the_flags_and_is_recorded(project):
    tmp_path, kins, _ = project
    fq = _fastq(6, seed=3)
    (tmp_path / "r.fq").write_bytes(fq)
    table = write_kin(tmp_path, "bait.fa", b">b\n" + fq.split(b"\n")[1] + b"\n", 7).path
    plain = kfilter.filter(str(tmp_path / "plain"), str(tmp_path / "r.fq"), [table], **FAKES)
    masked = kfilter.filter(str(tmp_path / "masked"), str(tmp_path / "r.fq"), [table], min_qual=41, **FAKES)
    assert plain["keep"][0] == 1 and masked["keep"][0] == 0                # every quality byte is below 33 + 41
    meta = json.load(open(str(tmp_path / "masked.kmf.json")))
    assert meta["min_qual"] == 41 and meta["qual_offset"] == 33


def test_refusals_come_before_any_file(project, capsys):
    tmp_path, kins, q = project
    fq1 = tmp_path / "a_1.fq"
    fq1.write_bytes(_fastq(6))
    fq2 = tmp_path / "a_2.fq"
    fq2.write_bytes(_fastq(5))
    cases = [(dict(min_hits=0), "min-hits"), (dict(min_percent=-1), "min-percent"), (dict(min_percent=101), "min-percent"),
             (dict(min_tables=3), "min-tables"), (dict(min_tables=0), "min-tables"), (dict(pair_rule="both"), "needs --mate"),
             (dict(min_qual=20), "FASTQ"), (dict(min_percent=2.5), "integer")]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            kfilter.filter(str(tmp_path / "bad"), q, kins, **kw, **FAKES)
    with pytest.raises(ValueError, match="same number of records.*6.*5"):
        kfilter.filter(str(tmp_path / "bad"), str(fq1), kins, mate=str(fq2), **FAKES)
    with pytest.raises(ValueError, match="does not exist"):
        kfilter.filter(str(tmp_path / "bad"), str(tmp_path / "missing.fa"), kins, **FAKES)
    for existing in ("bad.kept.fa", "bad.rest.fa", "bad.kmf", "bad.kmf.json"):
        (tmp_path / existing).write_bytes(b"mine")
        with pytest.raises(ValueError, match="already exists"):
            kfilter.filter(str(tmp_path / "bad"), q, kins, rest=True, **FAKES)
        assert (tmp_path / existing).read_bytes() == b"mine"
        (tmp_path / existing).unlink()
    assert not list(tmp_path.glob("bad*"))
    # the command line: `error: ...` and exit status 1, argparse's own refusals aside
    for argv in (["--min-hits", "0"], ["--min-percent", "101"], ["--min-tables", "3"], ["--pair-rule", "both"]):
        with pytest.raises(SystemExit) as exc:
            kfilter.main([str(tmp_path / "bad"), q] + kins + argv)
        assert exc.value.code == 1 and capsys.readouterr().err.startswith("error: ")
    assert not list(tmp_path.glob("bad*"))


def test_output_names():
    P = kfilter.output_paths
    assert {k: str(v) for k, v in P("p", "x.fa").items()} == {"kept": "p.kept.fa"}
    assert {k: str(v) for k, v in P("p", "x.fasta.gz", rest=True).items()} == {"kept": "p.kept.fa", "rest": "p.rest.fa"}
    assert {k: str(v) for k, v in P("p", "x.fq.bgz", mate="y.fq.bgz").items()} == {"kept_1": "p.kept_1.fq", "kept_2": "p.kept_2.fq"}
    assert list(P("p", "x.fastq", mate="y.fastq", rest=True)) == ["kept_1", "kept_2", "rest_1", "rest_2"]
    assert [str(v) for v in kfilter.kmf_paths("p")] == ["p.kmf", "p.kmf.json"]


def test_record_offsets_from_name_off():
    starts = kfilter.starts_from(np.array([30, 60, 61], dtype=np.uint64), 100)
    assert starts.dtype == np.uint64 and starts.tolist() == [29, 59, 60, 100]
    assert kfilter.starts_from(np.zeros(0, dtype=np.uint64), 7).tolist() == [7]
    assert filter_ref.record_starts_ref(FASTA).tolist() == [FASTA.index(b">  sp"), FASTA.index(b">none"), FASTA.index(b">short"),
                                                            FASTA.index(b">third"), FASTA.index(b">last"), len(FASTA)]


# ------------------------------------------------------------------ C-ABI surface ---------------
def test_select_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pykmer_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines()}
    lib = _lib.load()
    for name in SELECT_SYMBOLS:
        assert name in declared and name in exported and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "typedef struct pk_select pk_select;" in text and lib.pk_version() == 3
    assert hasattr(_lib, "Selector") and all(hasattr(_lib.Selector, m) for m in ("set_records", "feed", "feed_device", "finish", "__enter__"))


def test_select_refusals_need_no_device():
    lib = _lib.load()
    assert lib.pk_select_create(None, 0) == _lib.PK_ERR_ARG
    starts = np.array([0, 10, 9, 20], dtype=np.uint64)
    keep = np.ones(3, dtype=np.uint8)
    n_out = ctypes.c_uint64(7)
    buf = np.zeros(16, dtype=np.uint8)
    with _lib.Selector(0) as sel:
        assert lib.pk_select_set_records(sel._h, None, keep.ctypes.data, 3) == _lib.PK_ERR_ARG
        assert lib.pk_select_set_records(sel._h, starts.ctypes.data, None, 3) == _lib.PK_ERR_ARG
        assert lib.pk_select_set_records(None, starts.ctypes.data, keep.ctypes.data, 3) == _lib.PK_ERR_ARG
        with pytest.raises(ValueError, match=r"starts\[1\] = 10 is followed by 9"):
            sel.set_records(starts, keep)
        with pytest.raises(ValueError, match="offsets"):
            sel.set_records(starts[:3], keep)
        assert lib.pk_select_feed(sel._h, buf.ctypes.data, 16, buf.ctypes.data, 16, ctypes.byref(n_out)) == _lib.PK_ERR_STATE   # no records yet
        assert lib.pk_select_finish(sel._h, starts.ctypes.data) == _lib.PK_ERR_STATE
        assert lib.pk_select_finish(sel._h, None) == _lib.PK_ERR_ARG
    with _lib.Selector(0) as sel:                            # a stream without records needs no device either
        sel.set_records(np.array([5], dtype=np.uint64), np.zeros(0, dtype=np.uint8))
        assert sel.feed(b"0123456789").size == 0 and sel.feed(b"").size == 0
        assert lib.pk_select_feed(sel._h, buf.ctypes.data, 16, buf.ctypes.data, 16, None) == _lib.PK_ERR_ARG
        assert sel.finish() == {"bytes_fed": 10, "bytes_kept": 0, "records_kept": 0}
        with pytest.raises(_lib.PkError) as err:
            sel.feed(b"x")
        assert err.value.code == _lib.PK_ERR_STATE
