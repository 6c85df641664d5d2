"""CPU: the yardstick of the masked text (mask_ref) and what the GPU tests rely on, the host side of mask.py with the two
device passes stood in for by the yardstick, and the C-ABI surface of the cover and mask entry points."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import byte_inputs
import mask_inputs as mi
import mask_ref
import oracle
import query_coords_inputs as qci
import query_ref
from host_support import stage_host, write_kin
from pykmer_amd import _lib, mask, query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = mi.CHUNK
MASK_SYMBOLS = ("pk_query_set_cover", "pk_query_cover", "pk_query_set_mask", "pk_query_mask_text", "pk_query_mask_counts")


def _cases():
    """(name, text, k, tables, count window) of every stream the GPU tests compare."""
    out = []
    for k in mi.KS:
        for name, text in mi.texts(k):
            for window in mi.WINDOWS:
                out.append((f"{name}_k{k}_{window[0]}", text, k, mi.band_tables(k), window))
    around, edge = mi.seam_tables()
    out += [("seam_around", mi.seam_text(), mi.SEAM_K, [around], (1, 255)), ("seam_edge", mi.seam_text(), mi.SEAM_K, [edge], (1, 255)),
            ("hollow", mi.hollow()[0], mi.SEAM_K, [mi.hollow()[1]], (1, 255)),
            ("short_reads", qci.short_reads(), 5, mi.band_tables(5), (1, 255)),
            ("soup", byte_inputs.soup(31, 69_999), 5, query_ref.random_tables(5, 1, seed=1910), (255, 255)),
            ("line_starts", byte_inputs.line_start_fasta(), 5, query_ref.random_tables(5, 1, seed=1910), (255, 255))]
    return out


# ------------------------------------------------------------------ the yardstick ----------------
def test_consequences_of_the_definition_on_every_text():
    for name, text, k, tables, window in _cases():
        want = mask_ref.expected(text, k, tables, *window)
        fast = mask_ref.expected(text, k, tables, *window, fast=True)
        for key in ("base_off", "base_rec", "win_end", "cover", "bits"):                 # the two walkers agree
            assert np.array_equal(want[key], fast[key]), (name, key)
        n, cover = want["n_bases"], want["cover"]
        assert 0 < cover.sum() < n, name                     # covered and uncovered valid bases: no case passes by leaving one out
        body = np.frombuffer(text, dtype=np.uint8)
        assert np.isin(body[want["valid"]], np.frombuffer(b"ACGTacgt", dtype=np.uint8)).all() and want["valid"].sum() == n
        recs = oracle.kmer_list(text, k, records=True)[1]["records"]
        assert want["n_records"] == len(recs), name
        assert np.array_equal(mask_ref.unpack(want["bits"], n), cover) and want["bits"].size == (n + 7) // 8
        for invert in (False, True):
            soft, hard = mask_ref.masked_text(text, want, False, invert), mask_ref.masked_text(text, want, True, invert)
            s, h = np.frombuffer(soft, dtype=np.uint8), np.frombuffer(hard, dtype=np.uint8)
            assert len(soft) == len(hard) == len(text) and soft.upper() == text.upper(), name
            sel = np.zeros(len(text), dtype=bool)
            sel[want["base_off"][cover != invert]] = True
            assert not (sel & ~want["valid"]).any()
            assert np.array_equal(np.flatnonzero(h != body), np.flatnonzero(sel)), name   # every selected byte was a base, so none was N
            assert (h[sel] == ord("N")).all() and np.array_equal(np.flatnonzero(s != body), np.flatnonzero(sel & (body < 0x60))), name
            masked = mask_ref.masked_counts(want, invert)
            assert masked.dtype == np.uint64 and masked.shape == (want["n_records"],)
            assert int(masked.sum()) == (n - int(cover.sum()) if invert else int(cover.sum())), name


def _only_window_end(want, text_len):
    """Per valid base: the byte offset of the last base of its only matching window, or -1 if it lies in none or several."""
    k_of = want["k"]
    ends = want["win_end"][want["match"]]
    count = np.zeros(want["n_bases"] + 1, dtype=np.int64)
    np.add.at(count, ends - (k_of - 1), 1)
    np.add.at(count, ends + 1, -1)
    count = np.cumsum(count)[:want["n_bases"]]
    only = np.full(want["n_bases"], -1, dtype=np.int64)
    for e in ends:                                           # few matching windows in the seam inputs
        span = np.arange(e - k_of + 1, e + 1)
        only[span[count[span] == 1]] = want["base_off"][e]
    return only


def test_seam_inputs_hold_what_the_seam_tests_are_about():
    k, text = mi.SEAM_K, mi.seam_text()
    assert 2 * CHUNK < len(text) < 3 * CHUNK
    around, edge = mi.seam_tables()
    wa = mask_ref.expected(text, k, [around], 1, 255)
    in_reach = np.zeros(len(text), dtype=bool)
    for b in (CHUNK, 2 * CHUNK):
        in_reach[b - 450:b + 450] = True
    assert wa["cover"].sum() >= 2 * 700 and in_reach[wa["base_off"][wa["cover"]]].mean() > 0.75   # the matching windows are mostly those around the boundaries
    two = mask_ref.expected(text, k, [around], 2, 254)
    assert 0 < two["cover"].sum() < wa["cover"].sum()
    we = mask_ref.expected(text, k, [edge], 1, 255)
    we["k"] = k
    only = _only_window_end(we, len(text))
    off = we["base_off"]
    for b in (CHUNK, 2 * CHUNK):                             # a base whose only matching window ends in the next chunk
        assert ((off < b) & (only >= b)).any(), b
    cuts = mi.seam_cuts()
    assert cuts[0] == CHUNK - k - 2 and cuts[-1] == CHUNK + k + 2 and len(cuts) == 2 * k + 5
    held = [c for c in cuts if ((off < c) & (only >= c)).any()]                        # ... and one whose only matching window ends in the next feed
    assert len(held) >= k - 1, held
    wa["k"] = k
    only_a = _only_window_end(wa, len(text))
    assert any(((wa["base_off"] < c) & (only_a >= c)).any() for c in cuts) or wa["cover"][np.searchsorted(wa["base_off"], CHUNK) - 1]
    line = mi.line_cuts()
    assert len(line) == 62 and text[line[0] - 1:line[0]] == b"\n" and text[line[-1] - 1:line[-1]] == b"\n"


def test_hollow_and_long_inputs():
    k = mi.SEAM_K
    text, table = mi.hollow()
    want = mask_ref.expected(text, k, [table], 1, 255)
    off = want["base_off"]
    middle = (off >= CHUNK) & (off < 2 * CHUNK)
    assert middle.sum() == 3 < k - 1                          # fewer than k - 1 bases of the run in the middle chunk
    spans = [(off[e - k + 1], off[e]) for e in want["win_end"][want["match"]]]
    assert any(a < CHUNK and b >= 2 * CHUNK for a, b in spans)                          # a matching window's bases span three slots
    assert want["cover"][middle].all() and want["cover"][~middle].sum() > 16
    long_text, long_table = mi.long_text()
    assert 1024 * CHUNK < len(long_text) <= 1026 * CHUNK      # more chunks than one tile of the scans
    lw = mask_ref.expected(long_text, k, [long_table], 1, 255, fast=True)
    seam = 1024 * CHUNK
    near = (lw["base_off"] > seam - 100) & (lw["base_off"] < seam + 100)
    assert lw["cover"][near].all() and 0 < lw["cover"].sum() < lw["n_bases"] // 4


# ------------------------------------------------------------------ mask.py on the host ----------
FASTA = mi.TOOL_FASTA


def _text_of(path):
    import gzip
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


def _apply(query_file, cover, n_bases, out_file, hard=False, invert=False, device=0):
    text = _text_of(query_file)
    want = mask_ref.expected(text, 1, [np.ones(4, dtype=np.uint8)])
    assert want["n_bases"] == n_bases
    got = mask_ref.unpack(cover, n_bases)
    with mask.atomic_write(out_file, "wb") as fh:
        fh.write(mask_ref.masked_text(text, want, hard, invert, cover=got))
    masked = mask_ref.masked_counts(want, invert, cover=got)
    return {"masked": masked, "n_masked": int(masked.sum()), "n_records": want["n_records"], "bytes": len(text), "mask_s": 0.125}


FAKES = dict(run=_run, stage=stage_host, apply=_apply, hbm_budget=1 << 40)


@pytest.fixture()
def project(tmp_path):
    kins = [write_kin(tmp_path, "donor.fa", b">d\n" + mi.DONOR + b"\n", 5).path, write_kin(tmp_path, "host.fa", b">h\n" + mi.HOST + b"\n", 5).path]
    q = tmp_path / "contigs.fa"
    q.write_bytes(FASTA)
    return tmp_path, kins, str(q)


def test_mask_writes_the_three_files(project):
    tmp_path, kins, q = project
    tables = [np.fromfile(kin, dtype=np.uint8) for kin in kins]
    for n, (hard, invert) in enumerate(((False, False), (True, False), (False, True), (True, True))):
        proj = str(tmp_path / f"run{n}")
        res = mask.mask(proj, q, kins, min_count=1, max_count=254, hard=hard, invert=invert, **FAKES)
        want = mask_ref.expected(FASTA, 5, tables, 1, 254)
        assert 0 < want["cover"].sum() < want["n_bases"] and res["n_groups"] == 1
        assert sorted(p.name for p in tmp_path.glob(f"run{n}.*")) == [f"run{n}.kmm", f"run{n}.kmm.json", f"run{n}.masked.fa"]      # no .tmp
        assert (tmp_path / f"run{n}.masked.fa").read_bytes() == mask_ref.masked_text(FASTA, want, hard, invert)
        z = np.load(proj + ".kmm")
        assert sorted(z.files) == sorted(["masked", "n_valid", "seq_len", "kmer_len", "min_count", "max_count", "hard", "invert", "n_bases"])
        assert z["masked"].dtype == z["n_valid"].dtype == z["seq_len"].dtype == np.uint64
        assert np.array_equal(z["masked"], mask_ref.masked_counts(want, invert)) and int(z["n_bases"]) == want["n_bases"]
        assert (int(z["kmer_len"]), int(z["min_count"]), int(z["max_count"]), bool(z["hard"]), bool(z["invert"])) == (5, 1, 254, hard, invert)
        meta = json.load(open(proj + ".kmm.json"))
        for key in ("project_name", "kmer_len", "min_count", "max_count", "query_file", "records", "data"):      # the .kmq.json's
            assert key in meta
        n_masked = int(mask_ref.masked_counts(want, invert).sum())
        assert (meta["mode"], meta["invert"], meta["n_records"], meta["n_bases"], meta["n_masked"], meta["bytes"], meta["output"]) == \
            ("hard" if hard else "soft", invert, want["n_records"], want["n_bases"], n_masked, len(FASTA), proj + ".masked.fa")
        assert meta["lookup_s"] == 0.25 and meta["mask_s"] == 0.125 and meta["records"][0] == "donor piece" and len(meta["data"]) == 2
    two = mask.cover_bits(q, [query.load_header(kin) for kin in kins], 1, 254, run=_run, stage=stage_host, hbm_budget=4 ** 5 + 100)
    assert two["n_groups"] == 2 and two["lookup_s"] == 0.5 and np.array_equal(two["cover"], want["bits"])        # OR-ed over the groups


def test_last_line_of_the_tool(project, capsys, monkeypatch):
    tmp_path, kins, q = project
    monkeypatch.setattr(mask, "run_cover", _run)
    monkeypatch.setattr(mask, "stage_tables", lambda group, dev, threads: stage_host(group, dev))
    monkeypatch.setattr(mask, "apply_mask", _apply)
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(1 << 40))
    proj = str(tmp_path / "cli")
    mask.main([proj, q] + kins + ["--invert"])
    want = mask_ref.expected(FASTA, 5, [np.fromfile(kin, dtype=np.uint8) for kin in kins], 1, 255)
    last = capsys.readouterr().out.strip().split("\n")[-1]
    assert last == f"{want['n_bases'] - int(want['cover'].sum())} of {want['n_bases']} valid bases masked in {want['n_records']} records, {proj}.masked.fa"


def test_refusals_come_before_any_file(project, capsys):
    tmp_path, kins, q = project
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@r\nACGTACGT\n+\nIIIIIIII\n")
    bad = str(tmp_path / "bad")
    for name in ("reads.fq", "reads.fastq.gz", "reads.fq.bgz"):
        with pytest.raises(ValueError, match="filter.py"):
            mask.mask(bad, str(tmp_path / name), kins, **FAKES)
    cases = [(dict(min_count=0), "count window"), (dict(max_count=256), "count window"), (dict(min_count=9, max_count=3), "count window")]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            mask.mask(bad, q, kins, **kw, **FAKES)
    with pytest.raises(ValueError, match="at least one table"):
        mask.mask(bad, q, [], **FAKES)
    with pytest.raises(ValueError, match="does not exist"):
        mask.mask(bad, str(tmp_path / "missing.fa"), kins, **FAKES)
    with pytest.raises(ValueError, match="kin"):
        mask.mask(bad, q, [q], **FAKES)
    k7 = write_kin(tmp_path, "seven.fa", b">d\n" + mi.DONOR + b"\n", 7).path
    with pytest.raises(ValueError, match="kmer_len 7 differs"):
        mask.mask(bad, q, kins + [k7], **FAKES)
    for existing in ("bad.masked.fa", "bad.kmm", "bad.kmm.json"):
        (tmp_path / existing).write_bytes(b"mine")
        with pytest.raises(ValueError, match="already exists"):
            mask.mask(bad, q, kins, **FAKES)
        assert (tmp_path / existing).read_bytes() == b"mine"
        (tmp_path / existing).unlink()
    assert not list(tmp_path.glob("bad*"))
    # the command line: `error: ...` and exit status 1
    for argv in ([bad, str(fq)] + kins, [bad, q] + kins + ["--min-qual", "20"], [bad, q] + kins + ["--min-count", "0"]):
        with pytest.raises(SystemExit) as exc:
            mask.main(argv)
        assert exc.value.code == 1 and capsys.readouterr().err.startswith("error: ")
    assert not list(tmp_path.glob("bad*"))
    # bits of the wrong length never reach the device
    with pytest.raises(ValueError, match="bytes of cover bits"):
        mask.apply_mask(q, np.zeros(3, dtype=np.uint8), 100, tmp_path / "bad.fa")
    assert not list(tmp_path.glob("bad*"))
    assert [str(p) for p in mask.kmm_paths("p")] == ["p.masked.fa", "p.kmm", "p.kmm.json"]
    assert mask.count_bits(np.array([0xFF, 0xFF], dtype=np.uint8), 11) == 11


# ------------------------------------------------------------------ C-ABI surface ---------------
def test_mask_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pykmer_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines()}
    lib = _lib.load()
    for name in MASK_SYMBOLS:
        assert name in declared and name in exported and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "PK_MASK_HARD = 1" in text and "PK_MASK_INVERT = 2" in text and (_lib.MASK_HARD, _lib.MASK_INVERT) == (1, 2)
    assert lib.pk_version() == 3
    assert all(hasattr(_lib.QueryIndexer, m) for m in ("set_cover", "cover", "set_mask", "mask_text", "mask_counts"))
    assert _lib.QueryIndexer.TIMINGS[:7] == ("scan_s", "squeeze_s", "finalize_s", "zero_s", "feeds", "lookup_s", "coords_s") and \
        _lib.QueryIndexer.TIMINGS[7] == "mask_s"
    assert os.path.exists(os.path.join(ROOT, "mask.py")) and os.path.exists(os.path.join(ROOT, "pykmer_amd", "csrc", "kmer_cover.hip"))


def test_null_handles_are_argument_errors():
    lib = _lib.load()
    n = ctypes.c_uint64(0)
    buf = np.zeros(16, dtype=np.uint8)
    assert lib.pk_query_set_cover(None, 1) == _lib.PK_ERR_ARG
    assert lib.pk_query_cover(None, buf.ctypes.data, 128, ctypes.byref(n)) == _lib.PK_ERR_ARG
    assert lib.pk_query_set_mask(None, buf.ctypes.data, 128, 0) == _lib.PK_ERR_ARG
    assert lib.pk_query_mask_text(None, buf.ctypes.data, 16, ctypes.byref(n)) == _lib.PK_ERR_ARG
    assert lib.pk_query_mask_counts(None, buf.ctypes.data, 2, ctypes.byref(n)) == _lib.PK_ERR_ARG
