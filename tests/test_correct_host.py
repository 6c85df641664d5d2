"""CPU: the yardstick of correct.py (correct_ref) -- its address arithmetic against the oracle, hand-worked records, every
outcome class on random reads so that none can silently vanish from the GPU tests, planted errors restored at k = 15 -- and
the host side of correct.py with the device passes stood in for by the yardsticks, and the C-ABI surface of pk_correct."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import correct_inputs
import correct_ref
import fastq_ref
import mask_ref
import oracle
import query_ref
import trim_ref
from host_support import stage_host, write_kin
from pykmer_amd import _lib, correct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORRECT_SYMBOLS = ("pk_correct_create", "pk_correct_set_tables", "pk_correct_set_cover", "pk_correct_feed", "pk_correct_feed_device",
                   "pk_correct_finish", "pk_correct_timings", "pk_correct_destroy")
CLASSES = ("untried", "corrected", "ambiguous", "unfixable")


# ------------------------------------------------------------------ the reference alone ---------
@pytest.mark.parametrize("k", [5, 7, 15])
def test_address_is_the_oracles(k):
    rng = np.random.default_rng(k)
    seq = correct_inputs.LETTERS[rng.integers(0, 4, 200)].tobytes()
    codes = [correct_ref.CODE[c] for c in seq]
    mine = [correct_ref.address(codes[s:s + k]) for s in range(len(seq) - k + 1)]
    assert mine == oracle.kmer_list(b">s\n" + seq + b"\n", k).tolist()


def test_hand_worked_records():
    """k = 5, a genome of 40 bases as the table: one wrong base mid-read has exactly its own base as the one that passes; the
    same at position 1 has two windows (tried at M = 2, untried at the default 3); two errors k - 1 apart share a window and
    stay; two errors k apart are corrected both; an N next to the error takes windows away."""
    genome = b"ACGTTGCAAGGCTTAACCGGATATCGCGTAGCTAGGTCCA"
    table = oracle.count_fasta(b">g\n" + genome + b"\n", 5)["table"]

    def fq_of(read):
        return b"@r\n" + bytes(read) + b"\n+\n" + b"I" * len(read) + b"\n"

    def wrong(read, at):
        read[at] = ord("A") if read[at] != ord("A") else ord("C")

    read = bytearray(genome[:30])
    wrong(read, 14)
    want = correct_ref.expected(fq_of(read), 5, [table], M=1)
    assert (want["candidates"].tolist(), want["corrected"].tolist(), want["untried"].tolist()) == ([1], [1], [0])
    assert (want["fix_record"].tolist(), want["fix_pos"].tolist(), want["fix_old"].tolist(), want["fix_new"].tolist()) == ([0], [14], [read[14]], [genome[14]])
    assert want["patched"] == fq_of(genome[:30])
    lower = bytearray(read)
    lower[14] |= 0x20
    assert correct_ref.expected(fq_of(lower), 5, [table], M=1)["patched"] == fq_of(genome[:14] + bytes([genome[14] | 0x20]) + genome[15:30])   # case is kept
    read = bytearray(genome[:30])
    wrong(read, 1)
    for M, untried in ((2, 1), (None, 2)):                   # positions 0 and 1 are uncovered: one and two windows
        want = correct_ref.expected(fq_of(read), 5, [table], M=M)
        assert want["candidates"].tolist() == [2] and want["untried"].tolist() == [untried]
    assert correct_ref.expected(fq_of(read), 5, [table], M=2)["fix_pos"].tolist() == [1]
    for gap, fixed in ((4, 0), (5, 2)):
        read = bytearray(genome[:30])
        wrong(read, 10)
        wrong(read, 10 + gap)
        want = correct_ref.expected(fq_of(read), 5, [table], M=1)
        assert want["corrected"].tolist() == [fixed], gap
        assert (want["patched"] == fq_of(genome[:30])) == (fixed == 2)
    read = bytearray(genome[:30])
    wrong(read, 14)
    read[16] = ord("N")
    want = correct_ref.expected(fq_of(read), 5, [table], M=1)
    assert want["candidates"].tolist() == [2] and want["fix_pos"].tolist() == [14]       # 14 has the windows 10 and 11 of the run [0, 16), 15 has 11 alone
    assert correct_ref.expected(fq_of(read), 5, [table], M=3)["untried"].tolist() == [2]
    short = correct_ref.expected(fq_of(b"ACGT"), 5, [table], M=1)                          # shorter than k: no run, no candidate
    assert short["candidates"].tolist() == [0] and short["n_bases"] == 4


# seeds for which the assertions below hold (correct_inputs.tables(k, 1, seed), correct_inputs.random_reads(300, 80, seed + 1))
CLASS_SEEDS = {5: 905, 7: 907}


@pytest.mark.parametrize("k", [5, 7])
def test_every_class_occurs_on_random_reads(k):
    tabs, _ = correct_inputs.tables(k, 1, CLASS_SEEDS[k])
    held = np.count_nonzero(tabs[0]) / (4 ** k // 2)
    assert 0.4 < held < 0.6, held
    fq = correct_inputs.random_reads(300, 80, CLASS_SEEDS[k] + 1)
    for M in (1, 2, None):
        want = correct_ref.expected(fq, k, tabs, M=M)
        counts = {name: int(want[name].sum()) for name in CLASSES}
        print(k, M, counts)
        # M = 1: every candidate has a window, so none is untried, by the definition; M = 2: all four; the default: no ambiguous one is asked for
        for name in {1: CLASSES[1:], 2: CLASSES}.get(M, ("untried", "corrected", "unfixable")):
            assert counts[name] > 0, (k, M, counts)
        assert M != 1 or counts["untried"] == 0
        assert int(want["corrected"].sum()) == want["fix_record"].size


def test_inputs_hold_what_the_gpu_tests_rely_on():
    for k in (5, 7):
        tabs, genome = correct_inputs.tables(k, 3, seed=800 + k)
        union = np.zeros(4 ** k, dtype=bool)
        for t in tabs:
            union |= t != 0
        assert 0.4 < union.sum() / (4 ** k // 2) < 0.6
        fq = correct_inputs.stream(k, genome, seed=810 + k, final_newline=False, blank_tail=False)
        fastq_ref.fastq_to_fasta(fq)                         # well formed
        assert not fq.endswith((b"\n", b"\r"))
        tail = correct_inputs.stream(k, genome, seed=810 + k, blank_tail=True)
        assert tail.endswith(b"\n\r\n\n") and len(trim_ref.starts(tail)) == len(trim_ref.starts(fq))
        want = correct_ref.expected(tail, k, tabs, M=2)
        assert sorted(set(want["seq_len"].tolist())) == sorted(set(correct_inputs.lengths(k)))
        assert all(int(want[name].sum()) > 0 for name in CLASSES)
        fp = want["fix_pos"]
        assert ((fp >= 62) & (fp <= 65)).any() and (fp < k).any() and (fp >= 250).any()       # corrections at the seams of the 64-position steps
        assert any(np.count_nonzero(want["fix_record"] == r) >= 2 for r in set(want["fix_record"].tolist()))       # a read corrected twice
        other = correct_ref.expected(tail, k, tabs, 2, 254, M=2)                                   # the count window matters
        assert not np.array_equal(other["corrected"], want["corrected"])


def test_planted_errors_are_restored_at_k15():
    k = 15
    sources, sparse = query_ref.counted_case(k)
    clean = query_ref.reads_from(sources, k, 400, seed=77, fastq=True)
    fq, offs, olds = correct_inputs.plant(clean, 0.01, seed=78)
    assert offs.size > 20 and len(fq) == len(clean)
    want = correct_ref.expected(fq, k, sparse)
    assert int(want["corrected"].sum()) > 5 and int(want["ambiguous"].sum()) == 0
    at = (want["pos2"][want["fix_record"].astype(np.int64)] + want["fix_pos"]).astype(np.int64)
    assert np.isin(at, offs).all()                           # no correction where nothing was planted
    planted_old = dict(zip(offs.tolist(), olds.tolist()))
    assert [planted_old[a] for a in at.tolist()] == want["fix_new"].tolist()       # and every one restores the planted base
    patched = np.frombuffer(want["patched"], dtype=np.uint8)
    assert np.array_equal(patched[at], np.frombuffer(clean, dtype=np.uint8)[at])


# ------------------------------------------------------------------ fixes_from, validate_min_windows
def test_fixes_from_and_its_mismatch_error():
    a = b"@r\nACGT\n+\nIIII\n@s\n acgt\n+\n IIII\n"
    b = b"@r\nACTT\n+\nIIII\n@s\n acga\n+\n IIII\n"
    starts, pos2 = np.array([0, 15, 32], dtype=np.uint64), np.array([3, 19], dtype=np.uint64)
    rec, pos, old, new = correct.fixes_from(a, b, starts, pos2, corrected=np.array([1, 1], dtype=np.uint64))
    assert (rec.tolist(), pos.tolist(), bytes(old), bytes(new)) == ([0, 1], [2, 3], b"Gt", b"Ta")
    assert rec.dtype == pos.dtype == np.uint64 and old.dtype == new.dtype == np.uint8
    assert all(x.size == 0 for x in correct.fixes_from(a, a, starts, pos2, corrected=np.zeros(2, dtype=np.uint64)))
    with pytest.raises(ValueError, match="2 bytes differ"):
        correct.fixes_from(a, b, starts, pos2, corrected=np.array([1, 0], dtype=np.uint64))
    with pytest.raises(ValueError, match="bytes"):
        correct.fixes_from(a, b[:-1], starts, pos2)
    with pytest.raises(ValueError, match="outside the positions"):
        correct.fixes_from(a, b"@x" + a[2:], starts, pos2)


def test_validate_min_windows():
    assert correct.validate_min_windows(None, 15) == 8 and correct.validate_min_windows(None, 5) == 3 and correct.validate_min_windows(None, 17) == 9
    assert correct.validate_min_windows(1, 15) == 1 and correct.validate_min_windows(np.int64(15), 15) == 15
    for bad in (0, 16, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="--min-windows"):
            correct.validate_min_windows(bad, 15)
    assert correct_ref.default_min_windows(7) == correct.validate_min_windows(None, 7)
    assert [str(p) for p in correct.kme_paths("p")] == ["p.kme", "p.kme.json"] and str(correct.output_path("p")) == "p.corrected.fq"


# ------------------------------------------------------------------ correct.py through the hooks --
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


def _correct(reads_file, cover, n_bases, starts, ptrs, kmer_len, mn, mx, min_windows=None, min_qual=0, qual_offset=33, out_file=None, device=0):
    fq = _text_of(reads_file)
    assert np.array_equal(starts, trim_ref.starts(fq))
    want = correct_ref.expected(fq, kmer_len, ptrs, mn, mx, M=min_windows, T=min_qual + qual_offset if min_qual else 0,
                                cover=mask_ref.unpack(cover, n_bases))
    if out_file is not None:
        with correct.atomic_write(out_file, "wb") as fh:
            fh.write(want["patched"])
    return {**{key: want[key] for key in correct_ref.FIELDS + ("fix_record", "fix_pos", "fix_old", "fix_new")}, **correct_ref.totals(want),
            "bytes": len(fq), "correct_s": 0.125}


FAKES = dict(run=_run, stage=stage_host, correct=_correct, hbm_budget=1 << 40)


@pytest.fixture()
def project(tmp_path):
    genome = np.random.default_rng(4).integers(0, 4, 2500, dtype=np.uint8)
    fq, fa = fastq_ref.read_set(60, 60, seed=5, sub_rate=0.01, genome=genome)
    clean, _ = fastq_ref.read_set(60, 60, seed=5, sub_rate=0.0, genome=genome)
    kins = [write_kin(tmp_path, "reads.fa", fastq_ref.fastq_to_fasta(clean), 7).path,
            write_kin(tmp_path, "other.fa", b">o\n" + correct_inputs.LETTERS[np.random.default_rng(9).integers(0, 4, 300)].tobytes() + b"\n", 7).path]
    (tmp_path / "reads_1.fq").write_bytes(fq)
    return tmp_path, kins, str(tmp_path / "reads_1.fq"), fq


def _check_files(tmp_path, name, fq, want, k, mn, mx, M, reads_file):
    proj = str(tmp_path / name)
    assert sorted(p.name for p in tmp_path.glob(name + ".*")) == [name + ".corrected.fq", name + ".kme", name + ".kme.json"]     # no .tmp
    assert (tmp_path / (name + ".corrected.fq")).read_bytes() == want["patched"]
    z = np.load(proj + ".kme")
    assert sorted(z.files) == sorted(["candidates", "untried", "corrected", "ambiguous", "seq_len", "n_valid", "fix_record", "fix_pos", "fix_old",
                                      "fix_new", "kmer_len", "min_count", "max_count", "min_windows", "n_bases"])
    for key in ("candidates", "untried", "corrected", "ambiguous", "seq_len", "fix_record", "fix_pos"):
        assert z[key].dtype == np.uint64 and np.array_equal(z[key], want[key]), key
    assert z["n_valid"].dtype == np.uint64 and z["n_valid"].shape == want["seq_len"].shape
    for key in ("fix_old", "fix_new"):
        assert z[key].dtype == np.uint8 and np.array_equal(z[key], want[key]), key
    assert (int(z["kmer_len"]), int(z["min_count"]), int(z["max_count"]), int(z["min_windows"]), int(z["n_bases"])) == (k, mn, mx, M, want["n_bases"])
    meta = json.load(open(proj + ".kme.json"))
    for key in ("project_name", "kmer_len", "min_count", "max_count", "query_file", "data"):                   # the .kmq.json's, without records
        assert key in meta
    assert "records" not in meta
    t = correct_ref.totals(want)
    assert (meta["min_windows"], meta["n_records"], meta["n_candidates"], meta["n_untried"], meta["n_corrected"], meta["n_ambiguous"]) == \
        (M, t["n_records"], t["n_candidates"], t["n_untried"], t["n_corrected"], t["n_ambiguous"])
    assert meta["n_unfixable"] == int(want["unfixable"].sum()) and meta["n_reads_corrected"] == int((want["corrected"] > 0).sum())
    assert (meta["bytes"], meta["output"], meta["query_file"]) == (len(fq), proj + ".corrected.fq", reads_file)
    assert (meta["lookup_s"], meta["correct_s"]) == (0.25, 0.125)
    return meta


def test_correct_writes_its_files(project):
    tmp_path, kins, r1, fq = project
    tabs = [np.fromfile(kin, dtype=np.uint8) for kin in kins]
    res = correct.correct(str(tmp_path / "one"), r1, kins, **FAKES)
    want = correct_ref.expected(fq, 7, tabs)
    assert int(want["corrected"].sum()) > 0 and int(want["untried"].sum()) > 0
    meta = _check_files(tmp_path, "one", fq, want, 7, 1, 255, 4, r1)
    assert "min_qual" not in meta and res["n_corrected"] == int(want["corrected"].sum()) and len(meta["data"]) == 2
    # a second round over the output finds less to do, and indexer.py's reader takes the file
    fastq_ref.fastq_to_fasta((tmp_path / "one.corrected.fq").read_bytes())
    again = correct_ref.expected(want["patched"], 7, tabs)
    assert int(again["candidates"].sum()) < int(want["candidates"].sum())
    res = correct.correct(str(tmp_path / "two"), r1, kins[:1], min_count=1, max_count=254, min_windows=1, min_qual=10, **FAKES)
    want = correct_ref.expected(fq, 7, tabs[:1], 1, 254, M=1, T=43)
    meta = _check_files(tmp_path, "two", fq, want, 7, 1, 254, 1, r1)
    assert (meta["min_qual"], meta["qual_offset"]) == (10, 33) and want["n_bases"] < correct_ref.expected(fq, 7, tabs[:1], M=1)["n_bases"]


def test_last_line_of_the_tool(project, capsys, monkeypatch):
    tmp_path, kins, r1, fq = project
    monkeypatch.setattr(correct, "run_cover", _run)
    monkeypatch.setattr(correct, "stage_tables", lambda group, dev, threads: stage_host(group, dev))
    monkeypatch.setattr(correct, "correct_runs", _correct)
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(1 << 40))
    proj = str(tmp_path / "cli")
    correct.main([proj, r1] + kins + ["--min-windows", "2"])
    want = correct_ref.expected(fq, 7, [np.fromfile(kin, dtype=np.uint8) for kin in kins], M=2)
    last = capsys.readouterr().out.strip().split("\n")[-1]
    assert last == (f"{int(want['corrected'].sum())} bases corrected in {int((want['corrected'] > 0).sum())} of 60 reads "
                    f"({int(want['candidates'].sum())} candidates: {int(want['untried'].sum())} untried, {int(want['ambiguous'].sum())} ambiguous, "
                    f"{int(want['unfixable'].sum())} unfixable), {proj}.corrected.fq")


def test_refusals_come_before_any_file(project, capsys):
    tmp_path, kins, r1, fq = project
    bad = str(tmp_path / "bad")
    (tmp_path / "contigs.fa").write_bytes(b">c\nACGTACGTACGT\n")
    with pytest.raises(ValueError, match="FASTQ input"):
        correct.correct(bad, str(tmp_path / "contigs.fa"), kins, **FAKES)
    for kw, msg in ((dict(min_windows=0), "--min-windows"), (dict(min_windows=8), "--min-windows"), (dict(min_windows=2.5), "--min-windows"),
                    (dict(qual_offset=64), "--qual-offset belongs"), (dict(min_qual=20, qual_offset=50), "33 or 64"), (dict(min_count=0), "count window")):
        with pytest.raises(ValueError, match=msg):
            correct.correct(bad, r1, kins, **kw, **FAKES)
        assert not list(tmp_path.glob("bad*")), kw
    with pytest.raises(ValueError, match="staged together"):                     # a budget that holds one table of the two: named
        correct.correct(bad, r1, kins, **dict(FAKES, hbm_budget=4 ** 7 + 100))
    assert not list(tmp_path.glob("bad*"))
    with pytest.raises(ValueError, match="at least one table"):
        correct.correct(bad, r1, [], **FAKES)
    with pytest.raises(ValueError, match="does not exist"):
        correct.correct(bad, str(tmp_path / "missing.fq"), kins, **FAKES)
    for existing in ("bad.corrected.fq", "bad.kme", "bad.kme.json"):
        (tmp_path / existing).write_bytes(b"mine")
        with pytest.raises(ValueError, match="already exists"):
            correct.correct(bad, r1, kins, **FAKES)
        assert (tmp_path / existing).read_bytes() == b"mine"
        (tmp_path / existing).unlink()
    assert not list(tmp_path.glob("bad*"))
    for argv in ([bad, str(tmp_path / "contigs.fa")] + kins, [bad, r1] + kins + ["--min-windows", "0"], [bad, r1] + kins + ["--qual-offset", "33"]):
        with pytest.raises(SystemExit) as exc:
            correct.main(argv)
        assert exc.value.code == 1 and capsys.readouterr().err.startswith("error: ")
    assert not list(tmp_path.glob("bad*"))
    with pytest.raises(ValueError, match="bytes of cover bits"):                 # bits of the wrong length never reach the device
        correct.correct_runs(r1, np.zeros(3, dtype=np.uint8), 100, trim_ref.starts(fq), [1], 7)


def test_record_feeds_cut_the_stream_at_record_offsets(project, monkeypatch):
    """trim.RecordFeeds, the loop trim.py and correct.py share: every byte once, in order, whole records, the blank tail last."""
    from pykmer_amd import trim
    tmp_path, kins, r1, fq = project
    (tmp_path / "tail.fq").write_bytes(fq + b"\n\n")
    (tmp_path / "blank.fq").write_bytes(b"\n\r\n")
    monkeypatch.setattr(trim, "TRIM_FEED", 1 << 16)
    for name, text in (("reads_1.fq", fq), ("tail.fq", fq + b"\n\n"), ("blank.fq", b"\n\r\n")):
        starts = trim_ref.starts(text)
        feeds = trim.RecordFeeds(str(tmp_path / name), starts)
        got, n_records = [], 0
        for piece, offsets in feeds:
            assert int(offsets[-1]) == piece.size and (offsets.size == 1 or np.array_equal(offsets + np.uint64(len(b"".join(got))), starts[n_records:n_records + offsets.size]))
            got.append(piece.tobytes())
            n_records += offsets.size - 1
        feeds.check()
        assert b"".join(got) == text and n_records == len(starts) - 1
    with pytest.raises(ValueError, match="changed between the passes"):
        feeds = trim.RecordFeeds(str(tmp_path / "tail.fq"), trim_ref.starts(fq))
        list(feeds)
        feeds.check()


# ------------------------------------------------------------------ C-ABI surface ---------------
def test_correct_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pykmer_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines()}
    lib = _lib.load()
    for name in CORRECT_SYMBOLS:
        assert name in declared and name in exported and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "typedef struct pk_correct pk_correct;" in text and "PK_CORR_AMBIGUOUS = 5,\n       PK_CORR_FIELDS = 6" in text and lib.pk_version() == 3
    assert _lib.CORR_FIELDS == correct_ref.FIELDS and all(hasattr(_lib.Corrector, m) for m in ("set_tables", "set_cover", "feed", "feed_device", "finish", "timings"))
    assert os.path.exists(os.path.join(ROOT, "correct.py")) and os.path.exists(os.path.join(ROOT, "pykmer_amd", "csrc", "kmer_correct.hip"))


def test_correct_refusals_need_no_device():
    lib = _lib.load()
    one = np.zeros(16, dtype=np.uint64)
    assert lib.pk_correct_create(None, 5, 0) == _lib.PK_ERR_ARG
    h = _lib.ctypes.c_void_p()
    for k in (0, 4, 19, -1):
        assert lib.pk_correct_create(_lib.ctypes.byref(h), k, 0) == _lib.PK_ERR_ARG and not h
    assert lib.pk_correct_set_tables(None, one.ctypes.data, 1, 1, 255) == _lib.PK_ERR_ARG
    assert lib.pk_correct_set_cover(None, one.ctypes.data, 8, 0, 1) == _lib.PK_ERR_ARG
    assert lib.pk_correct_feed(None, one.ctypes.data, 8, one.ctypes.data, 0, one.ctypes.data, one.ctypes.data) == _lib.PK_ERR_ARG
    assert lib.pk_correct_finish(None, one.ctypes.data) == _lib.PK_ERR_ARG and lib.pk_correct_timings(None, one.ctypes.data) == _lib.PK_ERR_ARG
    with _lib.Corrector(5, 0) as c:
        for N, mn, mx in ((0, 1, 255), (17, 1, 255), (1, 0, 255), (1, 3, 2), (1, 1, 256)):
            assert lib.pk_correct_set_tables(c._h, one.ctypes.data, N, mn, mx) == _lib.PK_ERR_ARG
        assert lib.pk_correct_set_tables(c._h, None, 1, 1, 255) == _lib.PK_ERR_ARG
        assert lib.pk_correct_set_tables(c._h, one.ctypes.data, 1, 1, 255) == _lib.PK_ERR_ARG                   # a null table pointer
        assert lib.pk_correct_set_cover(c._h, one.ctypes.data, 8, 0, 1) == _lib.PK_ERR_STATE                   # no tables yet
        assert lib.pk_correct_feed(c._h, one.ctypes.data, 8, one.ctypes.data, 0, one.ctypes.data, one.ctypes.data) == _lib.PK_ERR_STATE
        assert lib.pk_correct_finish(c._h, one.ctypes.data) == _lib.PK_ERR_STATE and lib.pk_correct_finish(c._h, None) == _lib.PK_ERR_ARG
        with pytest.raises(ValueError, match="bytes of cover bits"):
            c.set_cover(np.zeros(3, dtype=np.uint8), 100)
