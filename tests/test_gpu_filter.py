"""GPU: filter.py end to end (pykmer_amd.filter over pk_query_* and pk_select_*) on tiny inputs at k = 5 and 7, against the
host restatements: query_ref for the hits, filter_ref for the rule, the record offsets and the selected bytes.  Every
written file is compared byte for byte."""
import gzip
import json
import os

import numpy as np
import pytest

import filter_ref
import query_ref
from fastq_qual_ref import mask_fastq_to_fasta
from gpu_support import run_py
from host_support import write_kin

pytestmark = pytest.mark.gpu

DONOR = b"TTGACCAGGTAACGTACGTTAGCACGTGGATCCAATTGGCACTGA"
HOST = b"GATTACAGATTACAGGTACCTTAGGCATCGATCGGATATCCGGA"

# wrapped lines, text before the first header, a header with leading blanks, records without a valid window, no final newline
FASTA = (b"; a comment line\n\n>  donor piece \t\n" + DONOR[:20] + b"\n" + DONOR[20:41] + b"\n>none\nNNNNNNNN\n>empty\n>tiny\nACG\n>host piece\n"
         + HOST[3:40] + b"\n>mixed\n" + DONOR[5:25] + b"N" + HOST[8:30] + b"\n>other\nCCCCCCCCCCCCAAAAAAAAAAAATTTT\n>last donor\n" + DONOR[10:])


def _fastq():
    """\\n, \\r\\n and lone \\r terminators, quality lines that begin with '@', a missing final newline."""
    reads = [(b"d0", DONOR[:30], b"\n"), (b"h0", HOST[:28], b"\r\n"), (b"d1 x", DONOR[12:], b"\r"), (b"n", b"NNNNNNNNNN", b"\n"),
             (b"h1", HOST[10:], b"\n"), (b"mix", DONOR[:12] + HOST[:12], b"\r\n")]
    out = []
    for i, (name, seq, nl) in enumerate(reads):
        qual = (b"@" if i % 2 == 0 else b"I") + b"I" * (len(seq) - 1)
        out.append(b"@" + name + nl + seq + nl + b"+" + nl + qual + nl)
    return b"".join(out)


FASTQ = _fastq()
FASTQ_OPEN = FASTQ[:-1]                                       # the last line without its terminator
FASTQ_BLANKS = FASTQ + b"\n\r\n\n"                            # blank lines behind the last record stay with it


@pytest.fixture(scope="module")
def tables(gpu, tmp_path_factory):
    """{k: ([donor.kin, host.kin], [donor table, host table])} at k = 5 and 7, indexed here."""
    d = tmp_path_factory.mktemp("filter_tables")
    out = {}
    for k in (5, 7):
        got = [write_kin(d, f"{name}{k}.fa", b">" + name.encode() + b"\n" + seq + b"\n", k) for name, seq in (("donor", DONOR), ("host", HOST))]
        out[k] = ([w.path for w in got], [w.table for w in got])
    return out


def _want(text, fmt, k, tabs, H=1, P=0, M=1, T=0):
    fasta_or_fastq = mask_fastq_to_fasta(text, T)[0] if T else text
    exp = query_ref.expected(fasta_or_fastq, k, tabs, 1, 255, "fasta" if T else fmt)
    matched = np.array(filter_ref.decide(exp["hits"], exp["n_valid"], H, P, M)[0], dtype=bool)
    return exp, matched, filter_ref.record_starts_ref(text, fmt)


def _forms(tmp_path, name, text):
    """The text as a plain, a gzip and a BGZF file."""
    from pykmer_amd import bgzf
    plain = tmp_path / name
    plain.write_bytes(text)
    gz = tmp_path / ("g_" + name + ".gz")
    with gzip.open(gz, "wb") as fh:
        fh.write(text)
    bgz = tmp_path / ("b_" + name)
    bgz.write_bytes(text)
    bgzf.compress_file(str(bgz), level=1)
    return [str(plain), str(gz), str(bgz) + ".bgz"]


@pytest.mark.parametrize("k", [5, 7])
@pytest.mark.parametrize("case", ["fasta", "fastq", "fastq_open", "fastq_blanks"])
def test_kept_and_rest_are_the_inputs_own_records(gpu, tables, tmp_path, case, k):
    from pykmer_amd import filter as kfilter
    text = {"fasta": FASTA, "fastq": FASTQ, "fastq_open": FASTQ_OPEN, "fastq_blanks": FASTQ_BLANKS}[case]
    fmt = "fasta" if case == "fasta" else "fastq"
    kins, tabs = tables[k]
    exp, matched, starts = _want(text, fmt, k, tabs[:1], H=3, P=40)
    assert matched.any() and not matched.all() and (exp["n_valid"] == 0).any()
    assert np.array_equal(kfilter.record_starts(_forms(tmp_path, "s." + ("fa" if fmt == "fasta" else "fq"), text)[0]), starts)
    for n, path in enumerate(_forms(tmp_path, "in." + ("fa" if fmt == "fasta" else "fq"), text)):
        for invert in (False, True):
            proj = str(tmp_path / f"p{n}{int(invert)}")
            res = kfilter.filter(proj, path, kins[:1], min_hits=3, min_percent=40, invert=invert, rest=True)
            keep = matched != invert
            assert np.array_equal(res["keep"], keep.astype(np.uint8)) and np.array_equal(res["starts"], starts)
            assert np.array_equal(res["hits"], exp["hits"]) and np.array_equal(res["n_valid"], exp["n_valid"])
            ext = "fa" if fmt == "fasta" else "fq"
            kept, rest = open(f"{proj}.kept.{ext}", "rb").read(), open(f"{proj}.rest.{ext}", "rb").read()
            assert kept == filter_ref.select_bytes(text, starts, keep) and rest == filter_ref.select_bytes(text, starts, ~keep)
            # kept and rest interleave back to the input's records
            pieces, ik, ir = [], 0, 0
            for r in range(len(keep)):
                ln = int(starts[r + 1] - starts[r])
                if keep[r]:
                    pieces.append(kept[ik:ik + ln])
                    ik += ln
                else:
                    pieces.append(rest[ir:ir + ln])
                    ir += ln
            assert b"".join(pieces) == text[int(starts[0]):] and ik == len(kept) and ir == len(rest)
            meta = json.load(open(proj + ".kmf.json"))
            assert meta["files"][0]["bytes_in"] == len(text) and meta["files"][0]["bytes_kept"] == len(kept) and meta["n_kept"] == int(keep.sum())
            assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]


def test_mates_and_pair_rules(gpu, tables, tmp_path):
    from pykmer_amd import filter as kfilter
    k = 7
    kins, tabs = tables[k]
    fq1 = FASTQ
    fq2 = FASTQ_OPEN.replace(DONOR[:30], HOST[2:32]).replace(HOST[10:], DONOR[4:38])     # read 0 turns host, read 4 donor
    p1, p2 = tmp_path / "r_1.fq", tmp_path / "r_2.fq"
    p1.write_bytes(fq1)
    p2.write_bytes(fq2)
    (_, m1, s1), (_, m2, s2) = _want(fq1, "fastq", k, tabs[:1], H=2), _want(fq2, "fastq", k, tabs[:1], H=2)
    assert (m1 | m2).sum() > (m1 & m2).sum() > 0
    for rule, flags in (("any", m1 | m2), ("both", m1 & m2)):
        proj = str(tmp_path / rule)
        res = kfilter.filter(proj, str(p1), kins[:1], min_hits=2, mate=str(p2), pair_rule=rule, rest=True)
        assert np.array_equal(res["keep"], flags.astype(np.uint8))
        for n, fq, starts in (("1", fq1, s1), ("2", fq2, s2)):
            assert open(f"{proj}.kept_{n}.fq", "rb").read() == filter_ref.select_bytes(fq, starts, flags)
            assert open(f"{proj}.rest_{n}.fq", "rb").read() == filter_ref.select_bytes(fq, starts, ~flags)
        z = np.load(proj + ".kmf")
        assert np.array_equal(z["match_2"][:, 0], m2.astype(np.uint8)) and np.array_equal(z["match"][:, 0], m1.astype(np.uint8))
    p3 = tmp_path / "short_2.fq"
    p3.write_bytes(fq2[:filter_ref.record_starts_ref(fq2, "fastq")[-2]])
    with pytest.raises(ValueError, match="same number of records"):
        kfilter.filter(str(tmp_path / "bad"), str(p1), kins[:1], mate=str(p3))
    assert not list(tmp_path.glob("bad*"))


def test_min_qual_changes_the_flags_and_no_byte(gpu, tables, tmp_path):
    from pykmer_amd import filter as kfilter
    k = 7
    kins, tabs = tables[k]
    # read 0 (donor) gets qualities below the threshold in its middle: masked it has too few hits, unmasked it matches
    lines = FASTQ.split(b"\n")
    lines[3] = b"@" + b"I" * 5 + b"#" * 20 + b"I" * 4
    fq = b"\n".join(lines)
    path = tmp_path / "q.fq"
    path.write_bytes(fq)
    (_, plain, starts), (_, masked, _) = _want(fq, "fastq", k, tabs[:1], H=8), _want(fq, "fastq", k, tabs[:1], H=8, T=33 + 20)
    assert plain[0] and not masked[0] and masked.any()
    a = kfilter.filter(str(tmp_path / "plain"), str(path), kins[:1], min_hits=8)
    b = kfilter.filter(str(tmp_path / "masked"), str(path), kins[:1], min_hits=8, min_qual=20)
    assert np.array_equal(a["keep"], plain.astype(np.uint8)) and np.array_equal(b["keep"], masked.astype(np.uint8))
    assert open(str(tmp_path / "plain.kept.fq"), "rb").read() == filter_ref.select_bytes(fq, starts, plain)
    assert open(str(tmp_path / "masked.kept.fq"), "rb").read() == filter_ref.select_bytes(fq, starts, masked)    # the input's own bytes: no N
    meta = json.load(open(str(tmp_path / "masked.kmf.json")))
    assert meta["min_qual"] == 20 and meta["qual_offset"] == 33


def test_two_table_groups_give_the_same_files(gpu, tables, tmp_path):
    from pykmer_amd import filter as kfilter
    k = 7
    kins, tabs = tables[k]
    path = tmp_path / "in.fa"
    path.write_bytes(FASTA)
    one = kfilter.filter(str(tmp_path / "one"), str(path), kins, min_tables=2, invert=True, hbm_budget=1 << 40)
    two = kfilter.filter(str(tmp_path / "two"), str(path), kins, min_tables=2, invert=True, hbm_budget=4 ** k + 100)
    assert one["n_groups"] == 1 and two["n_groups"] == 2
    exp, matched, starts = _want(FASTA, "fasta", k, tabs, M=2)
    assert matched.any() and np.array_equal(one["keep"], (~matched).astype(np.uint8))
    for key in ("keep", "match", "hits", "n_valid"):
        assert np.array_equal(one[key], two[key]), key
    assert open(str(tmp_path / "one.kept.fa"), "rb").read() == open(str(tmp_path / "two.kept.fa"), "rb").read() \
        == filter_ref.select_bytes(FASTA, starts, ~matched)


def test_select_records_with_flags_from_outside(gpu, tmp_path):
    from pykmer_amd import filter as kfilter
    for name, text, fmt in (("x.fa", FASTA, "fasta"), ("x.fq", FASTQ_BLANKS, "fastq")):
        path = tmp_path / name
        path.write_bytes(text)
        starts = filter_ref.record_starts_ref(text, fmt)
        keep = (np.arange(len(starts) - 1) % 3 != 1)
        done = kfilter.select_records(str(path), keep, tmp_path / ("out_" + name))
        want = filter_ref.select_bytes(text, starts, keep)
        assert (tmp_path / ("out_" + name)).read_bytes() == want
        assert {key: done[key] for key in ("n_records", "n_kept", "bytes_in", "bytes_kept")} == \
            {"n_records": keep.size, "n_kept": int(keep.sum()), "bytes_in": len(text), "bytes_kept": len(want)}
        with pytest.raises(ValueError, match="flags"):
            kfilter.select_records(str(path), keep[:-1], tmp_path / "never")
    assert not (tmp_path / "never").exists()


def test_cli(gpu, tables, tmp_path):
    k = 5
    kins, tabs = tables[k]
    path = tmp_path / "reads.fq.gz"
    with gzip.open(path, "wb") as fh:
        fh.write(FASTQ_BLANKS)
    proj = str(tmp_path / "cli")
    argv = ["filter.py", proj, str(path)] + kins + ["--min-hits", "4", "--min-percent", "30", "--invert", "--rest"]
    r = run_py(*argv, cwd=str(tmp_path))
    exp, matched, starts = _want(FASTQ_BLANKS, "fastq", k, tabs, H=4, P=30)
    assert matched.any() and not matched.all()
    kept = filter_ref.select_bytes(FASTQ_BLANKS, starts, ~matched)
    assert open(proj + ".kept.fq", "rb").read() == kept and open(proj + ".rest.fq", "rb").read() == filter_ref.select_bytes(FASTQ_BLANKS, starts, matched)
    last = r.stdout.strip().split("\n")[-1]
    assert last == f"{int((~matched).sum())} of {matched.size} records kept, {len(kept):,d} of {len(FASTQ_BLANKS):,d} bytes, {proj}.kept.fq {proj}.rest.fq"
    again = run_py(*argv, cwd=str(tmp_path), status=1)
    assert [ln for ln in again.stderr.split("\n") if ln.startswith("error: ") and "already exists" in ln]
    bad = run_py(*argv[:3], *kins, "--min-tables", "3", cwd=str(tmp_path), status=1)
    assert "min-tables" in bad.stderr


# ------------------------------------------------------------------ the product's size: reads at k = 15
@pytest.fixture(scope="module")
def tables15(gpu, tmp_path_factory):
    """([a.kin, b.kin], SparseTables) at k = 15: two 1 GiB tables of query_ref.counted_sources, written side by side."""
    from concurrent.futures import ThreadPoolExecutor
    d = tmp_path_factory.mktemp("filter_tables15")
    sources, sparse = query_ref.counted_case(15)
    with ThreadPoolExecutor(2) as pool:
        got = list(pool.map(lambda i: write_kin(d, f"t{i}.fa", sources[i], 15), range(2)))
    return [w.path for w in got], sparse[:2]


@pytest.mark.parametrize("form", ["plain", "gzip", "bgzf"])
def test_reads_at_k15_in_feeds_of_20011_bytes(gpu, tables15, tmp_path, monkeypatch, form):
    """5000 FASTQ reads of 0 .. 150 bases (tests/test_query_host.py checks the set) against two tables at k = 15, with the
    feeds of all three passes -- the query, record_starts and the selector -- cut every 20 011 bytes: inside headers, reads
    and quality lines, and more records than the record array first holds."""
    from pykmer_amd import filter as kfilter
    from pykmer_amd import indexer
    k = 15
    kins, tabs = tables15
    text = query_ref.reads_case(k, 5000, True)
    monkeypatch.setattr(indexer, "FEED_BYTES", 20_011)
    monkeypatch.setattr(indexer, "GZ_PIECE", 20_011)
    path = _forms(tmp_path, "reads.fq", text)[("plain", "gzip", "bgzf").index(form)]
    runs = [(False, 0), (True, 0)] + ([(False, 20)] if form == "plain" else [])
    for invert, Q in runs:
        exp, matched, starts = _want(text, "fastq", k, tabs, H=3, P=40, T=33 + Q if Q else 0)
        assert matched.any() and not matched.all() and (exp["n_valid"] == 0).any() and matched.size == 5000 > 4096
        proj = str(tmp_path / f"p{int(invert)}{Q}")
        res = kfilter.filter(proj, path, kins, min_hits=3, min_percent=40, invert=invert, rest=True, **({"min_qual": Q} if Q else {}))
        keep = matched != invert
        assert np.array_equal(res["keep"], keep.astype(np.uint8)) and np.array_equal(res["starts"], starts)
        assert np.array_equal(res["hits"], exp["hits"]) and np.array_equal(res["n_valid"], exp["n_valid"])
        kept, rest = open(f"{proj}.kept.fq", "rb").read(), open(f"{proj}.rest.fq", "rb").read()
        assert kept == filter_ref.select_bytes(text, starts, keep) and rest == filter_ref.select_bytes(text, starts, ~keep)
        pieces, ik, ir = [], 0, 0                            # kept and rest interleave back to the input
        for r in range(len(keep)):
            ln = int(starts[r + 1] - starts[r])
            if keep[r]:
                pieces.append(kept[ik:ik + ln])
                ik += ln
            else:
                pieces.append(rest[ir:ir + ln])
                ir += ln
        assert b"".join(pieces) == text and ik == len(kept) and ir == len(rest)
    if form == "plain":                                      # the masked run decides otherwise than the unmasked one
        assert not np.array_equal(matched, _want(text, "fastq", k, tabs, H=3, P=40)[1])
