"""CPU: the yardstick of the masked intervals (mask_bed_ref) against the other host restatements, the host side of
mask.py --bed with the device passes stood in for by the yardsticks, and the C-ABI surface of the interval entry points."""
import ctypes
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

import mask_bed_ref
import mask_inputs as mi
import mask_ref
import oracle
import query_coords_inputs as qci
import query_coords_ref
import query_ref
from host_support import stage_host, write_kin
from pykmer_amd import _lib, mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTERVAL_SYMBOLS = ("pk_query_set_intervals", "pk_query_interval_count", "pk_query_intervals")
# the `crlf` text of test_gpu_mask.py: lower case, CRLF, lone CR, dead text, no final newline
CRLF = (b"acgtACGTNN dead\r\n\r>r1 x\r\nACGTacgtNNacgtTTGACCA\rGGTCAttgacc  A\r\n\n>r2\nacgtacgtacgtTTGACCATGACGTA\r\n>r3\r\rTTGACGGTCATTGGTCA" * 40
        + b"\n>last\nACGTTGCAAGGTCATTGACC")


def _cases():
    """(name, text, k, tables, count window)"""
    out = [(name, text, 9, mi.band_tables(9), (2, 254)) for name, text in mi.texts(9)]
    random5 = query_ref.random_tables(5, 1, seed=1910)
    tool = [oracle.count_fasta(b">x\n" + seq + b"\n", 5)["table"] for seq in (mi.DONOR, mi.HOST)]
    out += [("blanks_k5", qci.blanks(), 5, random5, (255, 255)), ("tool", mi.TOOL_FASTA, 5, tool, (1, 255)), ("crlf", CRLF, 5, random5, (255, 255)),
            ("hollow", mi.hollow()[0], mi.SEAM_K, [mi.hollow()[1]], (1, 255))]
    return out


@pytest.mark.parametrize("name", [c[0] for c in _cases()])
def test_reference_intervals_on_every_text(name):
    _, text, k, tables, window = next(c for c in _cases() if c[0] == name)
    want = mask_ref.expected(text, k, tables, *window)
    rec_of, pos_of = mask_bed_ref.positions(text)
    # the two restatements of the position rule agree: the first base of every valid window
    seq_len, n_windows, starts = query_coords_ref.window_starts(text, k)
    first_base = want["base_off"][want["win_end"] - (k - 1)]
    assert np.array_equal(pos_of[first_base].astype(np.uint64), starts)
    assert np.array_equal(np.bincount(rec_of[first_base], minlength=want["n_records"]).astype(np.uint64), n_windows)
    assert (pos_of[want["valid"]] >= 0).all() and np.array_equal(rec_of[want["base_off"]], want["base_rec"])
    held = pos_of >= 0
    assert np.array_equal(np.bincount(rec_of[held], minlength=want["n_records"]).astype(np.uint64), seq_len)
    for invert in (False, True):
        sel = mask_bed_ref.selected_bytes(text, want, invert)
        rec, start, end = mask_bed_ref.intervals(text, sel)
        assert rec.size >= 1 and (want["valid"] & ~sel).any(), "a text without an interval, or without an unselected valid base"
        assert rec.dtype == start.dtype == end.dtype == np.uint64
        assert (start < end).all() and (end <= seq_len[rec.astype(np.int64)]).all()
        total = np.zeros(want["n_records"], dtype=np.uint64)
        np.add.at(total, rec.astype(np.int64), end - start)
        assert np.array_equal(total, mask_ref.masked_counts(want, invert))
        assert np.array_equal(mask_bed_ref.paint(text, rec, start, end), sel)
        same = rec[1:] == rec[:-1]
        assert (rec[1:] >= rec[:-1]).all() and (end[:-1][same] < start[1:][same]).all()          # ascending, and they never touch


def test_fast_reference_of_one_plain_record():
    text = qci.one_record()
    want = mask_ref.expected(text, mi.SEAM_K, [mi.seam_tables()[0]], 1, 255)
    slow = mask_bed_ref.intervals(text, mask_bed_ref.selected_bytes(text, want))
    fast = mask_bed_ref.intervals_one_plain_record(text, want, want["cover"])
    assert slow[0].size > 1 and all(np.array_equal(a, b) for a, b in zip(slow, fast))
    with pytest.raises(AssertionError):
        mask_bed_ref.intervals_one_plain_record(text.replace(b"A", b"N", 1), want, want["cover"])


# ------------------------------------------------------------------ mask.py --bed on the host ----
FASTA = mi.TOOL_FASTA


def _text_of(path):
    return (gzip.open if str(path).endswith(".gz") else open)(path, "rb").read()


def _run(query_file, kmer_len, ptrs, mn, mx, device, first):
    text = _text_of(query_file)
    want = mask_ref.expected(text, kmer_len, ptrs, mn, mx)
    exp = query_ref.expected(text, kmer_len, ptrs, mn, mx)
    out = {"seq_len": exp["seq_len"], "n_valid": exp["n_valid"], "cover": want["bits"], "n_bases": want["n_bases"], "n_bytes": len(text),
           "timings": {"lookup_s": 0.25}}
    if first:
        out["names"] = query_ref.names(text, exp["records"])
    return out


def _run_nothing(*args):
    out = _run(*args)
    out["cover"] = np.zeros_like(out["cover"])
    return out


CALLS = []


def _apply(query_file, cover, n_bases, out_file, hard=False, invert=False, device=0, intervals=False):
    CALLS.append(intervals)
    text = _text_of(query_file)
    want = mask_ref.expected(text, 1, [np.ones(4, dtype=np.uint8)])
    assert want["n_bases"] == n_bases
    got = mask_ref.unpack(cover, n_bases)
    with mask.atomic_write(out_file, "wb") as fh:
        fh.write(mask_ref.masked_text(text, want, hard, invert, cover=got))
    masked = mask_ref.masked_counts(want, invert, cover=got)
    out = {"masked": masked, "n_masked": int(masked.sum()), "n_records": want["n_records"], "bytes": len(text), "mask_s": 0.125}
    if intervals:
        rec, start, end = mask_bed_ref.intervals(text, mask_bed_ref.selected_bytes(text, want, invert, cover=got))
        out.update(iv_record=rec, iv_start=start, iv_end=end, n_intervals=int(rec.size), intervals_s=0.0625)
    return out


def _apply_without_intervals(query_file, cover, n_bases, out_file, hard=False, invert=False, device=0):
    """The hook of tests/test_mask_host.py: it takes no `intervals`."""
    return _apply(query_file, cover, n_bases, out_file, hard, invert, device)


FAKES = dict(run=_run, stage=stage_host, apply=_apply, hbm_budget=1 << 40)
KMM_KEYS = ["masked", "n_valid", "seq_len", "kmer_len", "min_count", "max_count", "hard", "invert", "n_bases"]
JSON_KEYS = ["project_name", "kmer_len", "min_count", "max_count", "query_file", "records", "data", "mode", "invert", "n_records", "n_bases", "n_masked",
             "bytes", "output", "lookup_s", "mask_s"]
CHROMS = ["donor", "none", "empty", "tiny", "host", "mixed", "other", "last"]


@pytest.fixture()
def project(tmp_path):
    kins = [write_kin(tmp_path, "donor.fa", b">d\n" + mi.DONOR + b"\n", 5).path, write_kin(tmp_path, "host.fa", b">h\n" + mi.HOST + b"\n", 5).path]
    q = tmp_path / "contigs.fa"
    q.write_bytes(FASTA)
    return tmp_path, kins, str(q)


def test_bed_names_and_write_bed(tmp_path):
    assert mask.bed_names(["donor piece", "x", "a\tb c"]) == ["donor", "x", "a"]
    assert mask.bed_names([n.strip() for n in query_ref.names(FASTA, oracle.kmer_list(FASTA, 5, records=True)[1]["records"])]) == CHROMS
    with pytest.raises(ValueError, match="record 2 has an empty header"):
        mask.bed_names(["a", ""])
    with pytest.raises(ValueError, match="records 1 and 3 both begin with 'a'"):
        mask.bed_names(["a x", "b", "a y"])
    u = np.array([0, 0, 2], dtype=np.uint64)
    mask.write_bed(tmp_path / "x.bed", ["c1", "c2", "cé"], u, np.array([0, 7, 1], dtype=np.uint64), np.array([3, 9, 2], dtype=np.uint64))
    assert (tmp_path / "x.bed").read_bytes() == "c1\t0\t3\nc1\t7\t9\ncé\t1\t2\n".encode("utf-8")
    assert [p.name for p in tmp_path.iterdir()] == ["x.bed"] and str(mask.bed_path("p")) == "p.masked.bed"


def test_mask_with_bed_writes_the_four_files(project):
    tmp_path, kins, q = project
    tables = [np.fromfile(kin, dtype=np.uint8) for kin in kins]
    for n, (hard, invert) in enumerate(((False, False), (True, True))):
        proj = str(tmp_path / f"run{n}")
        del CALLS[:]
        res = mask.mask(proj, q, kins, min_count=1, max_count=254, hard=hard, invert=invert, bed=True, **FAKES)
        assert CALLS == [True]
        want = mask_ref.expected(FASTA, 5, tables, 1, 254)
        assert sorted(p.name for p in tmp_path.glob(f"run{n}.*")) == [f"run{n}.kmm", f"run{n}.kmm.json", f"run{n}.masked.bed", f"run{n}.masked.fa"]
        rec, start, end = mask_bed_ref.intervals(FASTA, mask_bed_ref.selected_bytes(FASTA, want, invert))
        bed = (tmp_path / f"run{n}.masked.bed").read_bytes()
        assert rec.size >= 2 and bed == mask_bed_ref.bed_lines(CHROMS, rec, start, end)
        assert (tmp_path / f"run{n}.masked.fa").read_bytes() == mask_ref.masked_text(FASTA, want, hard, invert)
        z = np.load(proj + ".kmm")
        assert sorted(z.files) == sorted(KMM_KEYS + ["iv_record", "iv_start", "iv_end"])
        for key, ref in (("iv_record", rec), ("iv_start", start), ("iv_end", end)):
            assert z[key].dtype == np.uint64 and np.array_equal(z[key], ref) and np.array_equal(res[key], ref)
        meta = json.load(open(proj + ".kmm.json"))
        assert sorted(meta) == sorted(JSON_KEYS + ["bed", "n_intervals", "intervals_s"])
        assert (meta["bed"], meta["n_intervals"], meta["intervals_s"], meta["mask_s"]) == (proj + ".masked.bed", int(rec.size), 0.0625, 0.125)
    # by hand: the donor piece ("  donor piece \t") is 20 + 21 bases on two lines, the host piece 37 and the last donor 35, every
    # one in a window of its table; the N at position 20 of `mixed` parts the two runs around it; NNNNNNNN, the empty record,
    # ACG (shorter than a window) and the poly-C record hold no covered base
    assert (tmp_path / "run0.masked.bed").read_bytes() == b"donor\t0\t41\nhost\t0\t37\nmixed\t0\t20\nmixed\t21\t43\nlast\t0\t35\n"
    assert (tmp_path / "run1.masked.bed").read_bytes() == b"tiny\t0\t3\nother\t0\t28\n"


def test_without_bed_everything_is_as_before(project, capsys, monkeypatch):
    tmp_path, kins, q = project
    proj = str(tmp_path / "plain")
    del CALLS[:]
    res = mask.mask(proj, q, kins, **dict(FAKES, apply=_apply_without_intervals))
    assert CALLS == [False] and "iv_record" not in res and "bed" not in res
    assert sorted(p.name for p in tmp_path.glob("plain.*")) == ["plain.kmm", "plain.kmm.json", "plain.masked.fa"]
    assert sorted(np.load(proj + ".kmm").files) == sorted(KMM_KEYS) and sorted(json.load(open(proj + ".kmm.json"))) == sorted(JSON_KEYS)
    monkeypatch.setattr(mask, "run_cover", _run)
    monkeypatch.setattr(mask, "stage_tables", lambda group, dev, threads: stage_host(group, dev))
    monkeypatch.setattr(mask, "apply_mask", _apply)
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(1 << 40))
    want = mask_ref.expected(FASTA, 5, [np.fromfile(kin, dtype=np.uint8) for kin in kins], 1, 255)
    head = f"{int(want['cover'].sum())} of {want['n_bases']} valid bases masked in {want['n_records']} records, "
    mask.main([str(tmp_path / "cli0"), q] + kins)
    assert capsys.readouterr().out.strip().split("\n")[-1] == head + f"{tmp_path / 'cli0'}.masked.fa"
    mask.main([str(tmp_path / "cli1"), q] + kins + ["--bed"])
    n = mask_bed_ref.intervals(FASTA, mask_bed_ref.selected_bytes(FASTA, want))[0].size
    assert capsys.readouterr().out.strip().split("\n")[-1] == head + f"{tmp_path / 'cli1'}.masked.fa, {n} intervals in {tmp_path / 'cli1'}.masked.bed"


def test_an_empty_selection_gives_an_empty_bed(project):
    tmp_path, kins, q = project
    proj = str(tmp_path / "none")
    res = mask.mask(proj, q, kins, bed=True, **dict(FAKES, run=_run_nothing))
    assert res["n_masked"] == 0 and res["n_intervals"] == 0
    assert (tmp_path / "none.masked.bed").read_bytes() == b"" and (tmp_path / "none.masked.fa").read_bytes() == FASTA
    assert np.load(proj + ".kmm")["iv_start"].shape == (0,) and json.load(open(proj + ".kmm.json"))["n_intervals"] == 0


def test_bed_refusals_leave_no_file(project, capsys):
    tmp_path, kins, q = project
    bad = str(tmp_path / "bad")
    (tmp_path / "bad.masked.bed").write_bytes(b"mine")
    with pytest.raises(ValueError, match="already exists"):
        mask.mask(bad, q, kins, bed=True, **FAKES)
    assert (tmp_path / "bad.masked.bed").read_bytes() == b"mine"
    mask.mask(bad, q, kins, **FAKES)                         # without --bed the file is nobody's business
    for p in tmp_path.glob("bad*"):
        p.unlink()
    nameless = tmp_path / "nameless.fa"
    nameless.write_bytes(b">a\n" + mi.DONOR + b"\n>  \n" + mi.HOST + b"\n")
    twice = tmp_path / "twice.fa"
    twice.write_bytes(b">a x\n" + mi.DONOR + b"\n>b\nACGT\n>a y\n" + mi.HOST + b"\n")
    del CALLS[:]
    for src, msg in ((nameless, "record 2 has an empty header"), (twice, "records 1 and 3 both begin with 'a'")):
        with pytest.raises(ValueError, match=msg):
            mask.mask(bad, str(src), kins, bed=True, **FAKES)
        assert not list(tmp_path.glob("bad*"))
    assert CALLS == []                                       # refused between the phases
    mask.mask(bad, str(twice), kins, **FAKES)                # ... and only with --bed
    for p in tmp_path.glob("bad*"):
        p.unlink()
    with pytest.raises(SystemExit) as exc:                   # the command line: `error: ...` and exit status 1
        (tmp_path / "bad.masked.bed").write_bytes(b"mine")
        mask.main([bad, q] + kins + ["--bed"])
    assert exc.value.code == 1 and "already exists" in capsys.readouterr().err
    assert [p.name for p in tmp_path.glob("bad*")] == ["bad.masked.bed"]


# ------------------------------------------------------------------ C-ABI surface ---------------
def test_interval_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pykmer_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines()}
    lib = _lib.load()
    for name in INTERVAL_SYMBOLS:
        assert name in declared and name in exported and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.pk_version() == 3
    assert all(hasattr(_lib.QueryIndexer, m) for m in ("set_intervals", "intervals", "interval_seconds"))
    assert os.path.exists(os.path.join(ROOT, "pykmer_amd", "csrc", "kmer_intervals.hip"))


def test_null_handles_are_argument_errors():
    lib = _lib.load()
    n, s = ctypes.c_uint64(0), ctypes.c_double(0)
    buf = np.zeros(16, dtype=np.uint64)
    assert lib.pk_query_set_intervals(None, 1) == _lib.PK_ERR_ARG
    assert lib.pk_query_interval_count(None, ctypes.byref(n), ctypes.byref(s)) == _lib.PK_ERR_ARG
    assert lib.pk_query_intervals(None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 16) == _lib.PK_ERR_ARG
