"""CPU: the yardstick of trim.py (trim_ref) on hand-worked records, the segment layout against it, the decision, the host
side of trim.py with the device passes stood in for by the yardsticks, and the C-ABI surface of the pk_trim entry points."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import fastq_ref
import filter_ref
import mask_ref
import oracle
import query_ref
import trim_inputs
import trim_ref
from host_support import stage_host, write_kin
from pykmer_amd import _lib, trim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIM_SYMBOLS = ("pk_trim_create", "pk_trim_set_cover", "pk_trim_feed", "pk_trim_feed_device", "pk_trim_finish", "pk_trim_timings", "pk_trim_destroy")


def _bits(s: str) -> np.ndarray:
    return np.array([c == "1" for c in s], dtype=bool)


# (name, FASTQ, one cover bit per valid base, min_len, the kept runs, the trimmed file)
HAND = [
    ("error_base_mid_read", b"@r\nACGTACGTAC\n+\n0123456789\n", "1111011111", 1, [(5, 10)], b"@r\nCGTAC\n+\n56789\n"),
    ("tie_smallest_start", b"@r\nACGTACGTAC\n+\n0123456789\n", "1111011110", 1, [(0, 4)], b"@r\nACGT\n+\n0123\n"),
    ("run_at_the_left_end", b"@r\nACGTACGTAC\n+\n0123456789\n", "1111100000", 1, [(0, 5)], b"@r\nACGTA\n+\n01234\n"),
    ("run_at_the_right_end", b"@r\nACGTACGTAC\n+\n0123456789\n", "0000011111", 1, [(5, 10)], b"@r\nCGTAC\n+\n56789\n"),
    ("no_covered_base", b"@r\nACGT\n+\n0123\n@s\nAC\n+\nII\n", "000011", 1, [(0, 0), (0, 2)], b"@s\nAC\n+\nII\n"),
    ("too_short_for_min_len", b"@r\nACGTAC\n+\n012345\n@s\nACGTAC\n+\nIJKLMN\n", "111011" "111111", 4, [(0, 3), (0, 6)], b"@s\nACGTAC\n+\nIJKLMN\n"),
    ("empty_read", b"@e\n\n+\n\n@s\nAC\n+\nII\n", "11", 1, [(0, 0), (0, 2)], b"@s\nAC\n+\nII\n"),
    ("blanks_front_inside_behind", b"@b\n  AC GTAC \t\n+\nab0123456cd\n", "111111", 1, [(3, 7)], b"@b\nGTAC\n+\n3456\n"),
    ("blanks_whole_run", b"@b\n \tACGT \n+\nabIJKLc\n", "1111", 1, [(0, 4)], b"@b\nACGT\n+\nIJKL\n"),
    ("n_ends_a_run", b"@n\nACGNNACGTA\n+\n0123456789\n", "11111111", 1, [(5, 10)], b"@n\nACGTA\n+\n56789\n"),
    ("crlf", b"@c\r\nACGTAC\r\n+x\r\nIJKLMN\r\n", "011110", 1, [(1, 5)], b"@c\r\nCGTA\r\n+x\r\nJKLM\r\n"),
    ("lone_cr", b"@c\rACGTAC\r+\rIJKLMN\r", "011110", 1, [(1, 5)], b"@c\rCGTA\r+\rJKLM\r"),
    ("no_final_newline", b"@a\nACGT\n+\nIIII\n@z\nACGTAC\n+\nIJKLMN", "1111" "001111", 1, [(0, 4), (2, 6)], b"@a\nACGT\n+\nIIII\n@z\nGTAC\n+\nKLMN"),
    ("trailing_blank_lines", b"@t\nACGTAC\n+\nIJKLMN\n\n\r\n\n", "111100", 1, [(0, 4)], b"@t\nACGT\n+\nIJKL\n\n\r\n\n"),
    ("quality_begins_with_at", b"@q\nACGTAC\n+\n@JKLMN\n@r\nAC\n+\n@I\n", "011111" "11", 2, [(1, 6), (0, 2)], b"@q\nCGTAC\n+\nJKLMN\n@r\nAC\n+\n@I\n"),
]


def _layout(fq, want, keep):
    offsets, flags = trim.trim_segments(trim_ref.starts(fq), want, want["trim_start"], want["trim_end"], keep)
    assert offsets.dtype == np.uint64 and offsets.shape == (9 * len(keep) + 1,) and flags.shape == (9 * len(keep),)
    assert bool((offsets[1:] >= offsets[:-1]).all()) and int(offsets[0]) == 0 and int(offsets[-1]) == len(fq)
    return filter_ref.select_bytes(fq, offsets, flags)


@pytest.mark.parametrize("name,fq,cover,min_len,kept_runs,trimmed", HAND, ids=[c[0] for c in HAND])
def test_hand_worked_records(name, fq, cover, min_len, kept_runs, trimmed):
    want = trim_ref.runs(fq, _bits(cover))
    assert want["n_bases"] == len(cover)
    assert list(zip(want["trim_start"].tolist(), want["trim_end"].tolist())) == kept_runs
    keep = trim_ref.keep_of(want, min_len)
    assert np.array_equal(keep, trim.decide(want["trim_start"], want["trim_end"], min_len))
    assert trim_ref.trimmed_bytes(fq, want["trim_start"], want["trim_end"], keep) == trimmed
    assert _layout(fq, want, keep) == trimmed
    rest = trim_ref.rest_bytes(fq, keep)
    assert rest == filter_ref.select_bytes(fq, trim_ref.starts(fq), 1 - keep) and len(rest) + sum(
        int(b) - int(a) for a, b in zip(trim_ref.starts(fq)[:-1][keep != 0], trim_ref.starts(fq)[1:][keep != 0])) == len(fq)


def test_error_base_and_short_read_against_a_table():
    """The tables' way to the same bits at k = 5: one substituted base takes the k windows across it, so one position is
    lost and the longer side stays; a read shorter than k has no window, and every run is at least k long."""
    genome = b"ACGTTGCAAGGCTTAACCGGATATCGCGTAGCTAGGTCCA"
    table = oracle.count_fasta(b">g\n" + genome + b"\n", 5)["table"]
    read = bytearray(genome[:30])
    read[14] = ord("A") if read[14] != ord("A") else ord("C")
    fq = b"@hit\n" + bytes(read) + b"\n+\n" + bytes(range(40, 70)) + b"\n@short\nACGT\n+\nIIII\n"
    want = trim_ref.runs(fq, [table], 5)
    assert list(zip(want["trim_start"].tolist(), want["trim_end"].tolist())) == [(15, 30), (0, 0)] and want["covered"].tolist() == [29, 0]
    keep = trim_ref.keep_of(want, 5)
    assert keep.tolist() == [1, 0]
    assert trim_ref.trimmed_bytes(fq, want["trim_start"], want["trim_end"], keep) == b"@hit\n" + bytes(read[15:]) + b"\n+\n" + bytes(range(55, 70)) + b"\n"
    masked = trim_ref.runs(fq, [table], 5, T=50)             # qualities 40 .. 49 fall below the threshold byte 50: ten Ns in front
    assert list(zip(masked["trim_start"].tolist(), masked["trim_end"].tolist())) == [(15, 30), (0, 0)] and masked["covered"].tolist() == [15, 0]
    assert masked["n_bases"] == 20 + 4 and masked["seq_len"].tolist() == [30, 4]


@pytest.mark.parametrize("k,seed,final_newline", [(5, 1, True), (7, 2, False)])
def test_segments_give_the_trimmed_bytes_on_random_reads(k, seed, final_newline):
    fq = trim_inputs.stream(k, seed, reps=3, final_newline=final_newline)
    fastq_ref.fastq_to_fasta(fq)                             # well formed
    n_valid = np.bincount(mask_ref.walk(trim_ref.fasta_of(fq), 1)[1], minlength=len(trim_ref.starts(fq)) - 1)
    want = trim_ref.runs(fq, trim_inputs.bits(n_valid, seed))
    assert sorted(set(want["seq_len"].tolist())) == sorted(set(trim_inputs.lengths(k)))
    for min_len in (1, k, 40):
        keep = trim_ref.keep_of(want, min_len)
        assert 0 < keep.sum() < keep.size
        assert _layout(fq, want, keep) == trim_ref.trimmed_bytes(fq, want["trim_start"], want["trim_end"], keep)
    whole, cut, dropped = trim_ref.classes(want, k)
    assert min(whole, cut, dropped) >= 0.10, (whole, cut, dropped)


def test_decide_and_the_pair_rule():
    start, end = np.array([0, 3, 5, 0], dtype=np.uint64), np.array([0, 8, 9, 100], dtype=np.uint64)
    assert trim.decide(start, end, 1).tolist() == [0, 1, 1, 1] and trim.decide(start, end, 5).tolist() == [0, 1, 0, 1]
    assert trim.decide(start, end, 100).tolist() == [0, 0, 0, 1] and trim.decide(start, end, 101).tolist() == [0, 0, 0, 0]
    assert trim.decide(start, end, 5).dtype == np.uint8
    for bad in (0, -1, 2.5, True, "7"):
        with pytest.raises(ValueError, match="--min-len"):
            trim.decide(start, end, bad)
    assert trim.pair_keep([1, 1, 0, 0], [1, 0, 1, 0]).tolist() == [1, 0, 0, 0]
    with pytest.raises(ValueError, match="same number of records"):
        trim.pair_keep([1, 1], [1])
    assert {k: str(v) for k, v in trim.output_paths("p").items()} == {"trimmed": "p.trimmed.fq"}
    assert {k: str(v) for k, v in trim.output_paths("p", "m.fq", True).items()} == {
        "trimmed_1": "p.trimmed_1.fq", "trimmed_2": "p.trimmed_2.fq", "rest_1": "p.rest_1.fq", "rest_2": "p.rest_2.fq"}
    assert [str(p) for p in trim.kmt_paths("p")] == ["p.kmt", "p.kmt.json"]


# ------------------------------------------------------------------ trim.py through the hooks -----
def _text_of(path):
    return open(path, "rb").read()


def _run(reads_file, kmer_len, ptrs, mn, mx, device, first, min_qual_byte=0):
    fq = _text_of(reads_file)
    fasta = trim_ref.fasta_of(fq, min_qual_byte)
    want = mask_ref.expected(fasta, kmer_len, ptrs, mn, mx)
    exp = query_ref.expected(fasta, kmer_len, ptrs, mn, mx)
    out = {"seq_len": exp["seq_len"], "n_valid": exp["n_valid"], "cover": want["bits"], "n_bases": want["n_bases"], "n_bytes": len(fq),
           "name_off": trim_ref.starts(fq)[:-1] + np.uint64(1), "timings": {"lookup_s": 0.25}}
    if first:
        out["names"] = query_ref.names(fasta, exp["records"])
    return out


def _trim(reads_file, cover, n_bases, starts, min_qual=0, qual_offset=33, device=0):
    fq = _text_of(reads_file)
    assert np.array_equal(starts, trim_ref.starts(fq))
    want = trim_ref.runs(fq, mask_ref.unpack(cover, n_bases), T=min_qual + qual_offset if min_qual else 0)
    return {**{key: want[key] for key in trim_ref.FIELDS}, "n_records": len(starts) - 1, "n_covered": int(want["covered"].sum()), "trim_s": 0.125}


def _select(input_file, keep, out_file, starts=None, device=0):
    data = _text_of(input_file)
    out = filter_ref.select_bytes(data, starts, keep)
    with trim.atomic_write(out_file, "wb") as fh:
        fh.write(out)
    return {"n_records": len(keep), "n_kept": int(np.asarray(keep).sum()), "bytes_in": len(data), "bytes_kept": len(out), "select_s": 0.0625}


FAKES = dict(run=_run, stage=stage_host, trim=_trim, select=_select, hbm_budget=1 << 40)


@pytest.fixture()
def project(tmp_path):
    genome = np.random.default_rng(4).integers(0, 4, 500, dtype=np.uint8)
    fq, fa = fastq_ref.read_set(60, 60, seed=5, sub_rate=0.01, genome=genome)
    fq2, _ = fastq_ref.read_set(60, 60, seed=6, sub_rate=0.01, genome=genome)
    kin = write_kin(tmp_path, "reads.fa", fa, 7).path
    (tmp_path / "reads_1.fq").write_bytes(fq)
    (tmp_path / "reads_2.fq").write_bytes(fq2)
    return tmp_path, [kin], str(tmp_path / "reads_1.fq"), str(tmp_path / "reads_2.fq"), fq, fq2


def test_trim_writes_its_files(project):
    tmp_path, kins, r1, r2, fq, fq2 = project
    table = np.fromfile(kins[0], dtype=np.uint8)
    proj = str(tmp_path / "one")
    res = trim.trim(proj, r1, kins, min_count=2, min_len=40, rest=True, **FAKES)
    want = trim_ref.runs(fq, [table], 7, 2, 255)
    keep = trim_ref.keep_of(want, 40)
    assert min(trim_ref.classes(want, 40)) >= 0.10
    assert sorted(p.name for p in tmp_path.glob("one.*")) == ["one.kmt", "one.kmt.json", "one.rest.fq", "one.trimmed.fq"]      # no .tmp
    trimmed, rest = (tmp_path / "one.trimmed.fq").read_bytes(), (tmp_path / "one.rest.fq").read_bytes()
    assert trimmed == trim_ref.trimmed_bytes(fq, want["trim_start"], want["trim_end"], keep) and rest == trim_ref.rest_bytes(fq, keep)
    # trimmed and rest together hold every record once, in order within each file
    names = [fq[a + 1:fq.index(b"\n", a)] for a in trim_ref.starts(fq)[:-1].tolist()]
    got = [[t[a + 1:t.index(b"\n", a)] for a in trim_ref.starts(t)[:-1].tolist()] for t in (trimmed, rest)]
    assert got[0] == [n for n, f in zip(names, keep) if f] and got[1] == [n for n, f in zip(names, keep) if not f]
    fastq_ref.fastq_to_fasta(trimmed)                        # still FASTQ: line 4 is as long as line 2
    z = np.load(proj + ".kmt")
    assert sorted(z.files) == sorted(["trim_start", "trim_end", "covered", "seq_len", "n_valid", "keep", "kmer_len", "min_count", "max_count",
                                      "min_len", "n_bases"])
    for key in ("trim_start", "trim_end", "covered", "seq_len"):
        assert z[key].dtype == np.uint64 and np.array_equal(z[key], want[key]), key
    assert z["keep"].dtype == np.uint8 and np.array_equal(z["keep"], keep) and z["n_valid"].dtype == np.uint64
    assert (int(z["kmer_len"]), int(z["min_count"]), int(z["max_count"]), int(z["min_len"]), int(z["n_bases"])) == (7, 2, 255, 40, want["n_bases"])
    meta = json.load(open(proj + ".kmt.json"))
    for key in ("project_name", "kmer_len", "min_count", "max_count", "query_file", "data"):                   # the .kmq.json's, without records
        assert key in meta
    assert "records" not in meta and "min_qual" not in meta
    length = (want["trim_end"] - want["trim_start"]).astype(np.int64)
    assert (meta["min_len"], meta["mate_file"], meta["n_records"], meta["n_kept"], meta["bases_in"], meta["bases_kept"]) == \
        (40, None, 60, int(keep.sum()), int(want["seq_len"].sum()), int(length[keep != 0].sum()))
    assert meta["n_trimmed"] == int(((keep != 0) & (length < want["seq_len"].astype(np.int64))).sum()) == res["n_trimmed"]
    assert meta["outputs"] == [proj + ".trimmed.fq", proj + ".rest.fq"] and [f["role"] for f in meta["files"]] == ["trimmed", "rest"]
    assert meta["files"][0] == {"role": "trimmed", "file": proj + ".trimmed.fq", "input": r1, "n_records": 60, "n_kept": int(keep.sum()),
                                "bytes_in": len(fq), "bytes_kept": len(trimmed)}
    assert meta["files"][1]["n_kept"] == 60 - int(keep.sum()) and meta["files"][1]["bytes_kept"] == len(rest)
    assert (meta["lookup_s"], meta["trim_s"], meta["select_s"]) == (0.25, 0.125, 0.125)
    # the default --min-len is kmer_len: exactly the reads with a matching window
    res = trim.trim(str(tmp_path / "dflt"), r1, kins, min_count=2, **FAKES)
    assert res["min_len"] == 7 and np.array_equal(res["keep"], (want["covered"] > 0).astype(np.uint8))


def test_mate_rest_and_min_qual(project):
    tmp_path, kins, r1, r2, fq, fq2 = project
    table = np.fromfile(kins[0], dtype=np.uint8)
    proj = str(tmp_path / "pair")
    res = trim.trim(proj, r1, kins, min_len=12, mate=r2, rest=True, min_qual=10, **FAKES)
    w1, w2 = trim_ref.runs(fq, [table], 7, T=43), trim_ref.runs(fq2, [table], 7, T=43)
    keep = trim_ref.keep_of(w1, 12) & trim_ref.keep_of(w2, 12)
    assert 0 < keep.sum() < keep.size and (trim_ref.keep_of(w1, 12) != trim_ref.keep_of(w2, 12)).any()
    assert sorted(p.name for p in tmp_path.glob("pair.*")) == ["pair.kmt", "pair.kmt.json", "pair.rest_1.fq", "pair.rest_2.fq", "pair.trimmed_1.fq",
                                                               "pair.trimmed_2.fq"]
    for tag, text, w in (("1", fq, w1), ("2", fq2, w2)):
        assert (tmp_path / f"pair.trimmed_{tag}.fq").read_bytes() == trim_ref.trimmed_bytes(text, w["trim_start"], w["trim_end"], keep)
        assert (tmp_path / f"pair.rest_{tag}.fq").read_bytes() == trim_ref.rest_bytes(text, keep)
    z = np.load(proj + ".kmt")
    assert {"trim_start_2", "trim_end_2", "covered_2", "seq_len_2", "n_valid_2", "n_bases_2"} <= set(z.files) and "keep_2" not in z.files
    assert np.array_equal(z["keep"], keep) and np.array_equal(z["trim_end_2"], w2["trim_end"]) and int(z["n_bases_2"]) == w2["n_bases"]
    meta = json.load(open(proj + ".kmt.json"))
    assert (meta["min_qual"], meta["qual_offset"], meta["mate_file"], meta["n_kept"]) == (10, 33, r2, int(keep.sum()))
    assert [f["role"] for f in meta["files"]] == ["trimmed_1", "trimmed_2", "rest_1", "rest_2"] and meta["files"][1]["input"] == r2
    assert meta["bases_in"] == int(w1["seq_len"].sum() + w2["seq_len"].sum()) and res["lookup_s"] == 0.5


def test_last_line_of_the_tool(project, capsys, monkeypatch):
    tmp_path, kins, r1, r2, fq, fq2 = project
    monkeypatch.setattr(trim, "run_cover", _run)
    monkeypatch.setattr(trim, "stage_tables", lambda group, dev, threads: stage_host(group, dev))
    monkeypatch.setattr(trim, "trim_runs", _trim)
    monkeypatch.setattr(trim, "select_records", _select)
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(1 << 40))
    proj = str(tmp_path / "cli")
    trim.main([proj, r1] + kins + ["--min-count", "2", "--min-len", "40"])
    want = trim_ref.runs(fq, [np.fromfile(kins[0], dtype=np.uint8)], 7, 2, 255)
    keep = trim_ref.keep_of(want, 40) != 0
    length = (want["trim_end"] - want["trim_start"]).astype(np.int64)
    last = capsys.readouterr().out.strip().split("\n")[-1]
    assert last == (f"{int(keep.sum())} of 60 reads kept, {int((keep & (length < want['seq_len'].astype(np.int64))).sum())} of them trimmed, "
                    f"{int(length[keep].sum()):,d} of {int(want['seq_len'].sum()):,d} bases, {proj}.trimmed.fq")


def test_refusals_come_before_any_file(project, capsys):
    tmp_path, kins, r1, r2, fq, fq2 = project
    bad = str(tmp_path / "bad")
    (tmp_path / "contigs.fa").write_bytes(b">c\nACGTACGTACGT\n")
    (tmp_path / "fewer.fq").write_bytes(fq2[:int(trim_ref.starts(fq2)[59])])
    with pytest.raises(ValueError, match="mask.py"):
        trim.trim(bad, str(tmp_path / "contigs.fa"), kins, **FAKES)
    with pytest.raises(ValueError, match="mask.py"):
        trim.trim(bad, r1, kins, mate=str(tmp_path / "contigs.fa"), **FAKES)
    for kw, msg in ((dict(min_len=0), "--min-len"), (dict(min_len=2.5), "--min-len"), (dict(qual_offset=64), "--qual-offset belongs"),
                    (dict(min_qual=20, qual_offset=50), "33 or 64"), (dict(min_count=0), "count window"),
                    (dict(mate=str(tmp_path / "fewer.fq"), rest=True), "same number of records")):
        with pytest.raises(ValueError, match=msg):
            trim.trim(bad, r1, kins, **kw, **FAKES)
        assert not list(tmp_path.glob("bad*")), kw
    with pytest.raises(ValueError, match="at least one table"):
        trim.trim(bad, r1, [], **FAKES)
    with pytest.raises(ValueError, match="does not exist"):
        trim.trim(bad, str(tmp_path / "missing.fq"), kins, **FAKES)
    for existing in ("bad.trimmed.fq", "bad.rest.fq", "bad.kmt", "bad.kmt.json"):
        (tmp_path / existing).write_bytes(b"mine")
        with pytest.raises(ValueError, match="already exists"):
            trim.trim(bad, r1, kins, rest=True, **FAKES)
        assert (tmp_path / existing).read_bytes() == b"mine"
        (tmp_path / existing).unlink()
    assert not list(tmp_path.glob("bad*"))
    for argv in ([bad, str(tmp_path / "contigs.fa")] + kins, [bad, r1] + kins + ["--min-len", "0"], [bad, r1] + kins + ["--qual-offset", "33"]):
        with pytest.raises(SystemExit) as exc:
            trim.main(argv)
        assert exc.value.code == 1 and capsys.readouterr().err.startswith("error: ")
    assert not list(tmp_path.glob("bad*"))
    with pytest.raises(ValueError, match="bytes of cover bits"):                 # bits of the wrong length never reach the device
        trim.trim_runs(r1, np.zeros(3, dtype=np.uint8), 100, trim_ref.starts(fq))


# ------------------------------------------------------------------ C-ABI surface ---------------
def test_trim_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pykmer_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines()}
    lib = _lib.load()
    for name in TRIM_SYMBOLS:
        assert name in declared and name in exported and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "typedef struct pk_trim pk_trim;" in text and "PK_TRIM_LEAD = 8, PK_TRIM_FIELDS = 9" in text and lib.pk_version() == 3
    assert _lib.TRIM_FIELDS == trim_ref.FIELDS and all(hasattr(_lib.Trimmer, m) for m in ("set_cover", "feed", "feed_device", "finish", "timings"))
    assert os.path.exists(os.path.join(ROOT, "trim.py")) and os.path.exists(os.path.join(ROOT, "pykmer_amd", "csrc", "kmer_trim.hip"))


def test_trim_refusals_need_no_device():
    lib = _lib.load()
    one = np.zeros(16, dtype=np.uint64)
    assert lib.pk_trim_create(None, 0) == _lib.PK_ERR_ARG
    assert lib.pk_trim_set_cover(None, one.ctypes.data, 8, 0) == _lib.PK_ERR_ARG
    assert lib.pk_trim_feed(None, one.ctypes.data, 8, one.ctypes.data, 0, one.ctypes.data) == _lib.PK_ERR_ARG
    assert lib.pk_trim_finish(None, one.ctypes.data) == _lib.PK_ERR_ARG and lib.pk_trim_timings(None, one.ctypes.data) == _lib.PK_ERR_ARG
    with _lib.Trimmer(0) as t:
        assert lib.pk_trim_set_cover(t._h, None, 8, 0) == _lib.PK_ERR_ARG
        assert lib.pk_trim_set_cover(t._h, one.ctypes.data, 8, 256) == _lib.PK_ERR_ARG
        assert lib.pk_trim_feed(t._h, one.ctypes.data, 8, one.ctypes.data, 0, one.ctypes.data) == _lib.PK_ERR_STATE      # no cover bits yet
        assert lib.pk_trim_finish(t._h, one.ctypes.data) == _lib.PK_ERR_STATE and lib.pk_trim_finish(t._h, None) == _lib.PK_ERR_ARG
        with pytest.raises(ValueError, match="bytes of cover bits"):
            t.set_cover(np.zeros(3, dtype=np.uint8), 100)
