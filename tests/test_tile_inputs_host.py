"""Host checks of the scan-tile seam inputs (inputs.tile_seam_fasta, fastq_ref.seam_read_set), from the oracle alone: every
site is what it claims to be, and losing the parser state at its byte B changes the answer -- counting text[:B] and
text[B:] apart (offsets and record numbers of each part its own, tables added) differs from counting the text.  A site
for which it does not tests nothing on the GPU (tests/test_gpu_tiles.py)."""
import functools

import numpy as np
import pytest

import fastq_ref
import inputs
import oracle
import slice_ref

CHUNK = 16384
TILE = inputs.TILE


def _count(data, k: int, table: bool = False):
    """oracle.count_fasta; without the table: the same pass of the oracle with no table and no k-mer list to write."""
    if table:
        return oracle.count_fasta(data, k)
    import ctypes
    buf = np.frombuffer(data, dtype=np.uint8)
    nk, bp, nr = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    recs = np.zeros(data.count(b">") + 1, dtype=oracle.RECORD_DTYPE)
    rc = oracle._load().pko_count_fasta_ex(buf.ctypes.data, buf.size, k, None, ctypes.byref(nk), ctypes.byref(bp), recs.ctypes.data,
                                           recs.size, ctypes.byref(nr), None, 0)
    assert rc == 0 and nr.value <= recs.size
    return {"num_kmers": int(nk.value), "total_bp": int(bp.value), "records": recs[:nr.value].copy()}


def _split_differs(text: bytes, whole: dict, k: int, B: int) -> bool:
    """Does the count of text[:B] and text[B:], each on its own, differ from the count of the text?  The tables are
    counted only where the totals and the records do not already decide it."""
    a, b = _count(text[:B], k), _count(text[B:], k)
    if a["num_kmers"] + b["num_kmers"] != whole["num_kmers"]:
        return True
    if not np.array_equal(np.concatenate([a["records"], b["records"]]), whole["records"]):
        return True
    assert k <= 11, "totals and records agree: the tables have to decide, run this site at a small k"
    tables = [oracle.count_fasta(t, k)["table"] for t in (text[:B], text[B:], text)]
    return not np.array_equal(np.minimum(tables[0].astype(np.uint16) + tables[1], 255).astype(np.uint8), tables[2])


def _crossing(text: bytes, k: int, B: int) -> int:
    """slice_ref.crossing_windows at B, on the text from a line start four chunks in front of the site (under a header of its
    own) to 120 000 bytes behind it: the windows that cross B lie inside."""
    lo = text.index(b"\n", B - 4 * CHUNK) + 1
    assert lo < B - 2 * CHUNK - 100 and text[lo] in b"ACGT"
    return slice_ref.crossing_windows(b">x\n" + text[lo:B + 120_000], k, B - lo + 3)


def _plain(text: bytes, lo: int, hi: int) -> bool:
    """text[lo:hi] is ordinary sequence lines: bases and newlines only, no line of more than 60 bases."""
    part = np.frombuffer(text, dtype=np.uint8)[max(lo, 0):hi]
    nl = np.flatnonzero(part == 10)
    return bool(np.isin(part, np.frombuffer(b"ACGT\n", dtype=np.uint8)).all()) and nl.size >= 2 and int(np.diff(nl).max()) <= 61 \
        and int(np.diff(nl).min()) >= 2


def _oldest_crossing_start(text: bytes, B: int, n_before: int) -> int:
    """Offset of the base that has n_before - 1 bases between itself and B (line terminators and blanks skipped)."""
    at = B
    while n_before:
        at -= 1
        n_before -= text[at] in b"ACGT"
    return at


def _check_sites(text: bytes, sites, plan: dict, k: int, gap_chunks: int = 16):
    assert not text.endswith(b"\n") and text.startswith(inputs.TILE_HEADER)
    whole = _count(text, k)
    recs = whole["records"]
    for site in sites:
        kind, d, B = site
        p = plan[site]
        assert _crossing(text, k, B) == p["crossing"], site
        lo, hi = p["span"]
        assert lo <= B <= hi
        assert _plain(text, B - 16 * CHUNK if gap_chunks >= 16 else lo - gap_chunks * CHUNK, lo) and text[lo - 1] == 10, site
        assert _plain(text, hi, min(hi + min(gap_chunks, 16) * CHUNK, len(text) - 57)) and text[hi - 1] == 10, site
        for name_off, name, seq_len in p["records"]:
            i = int(np.searchsorted(recs["name_off"], name_off))
            assert i < len(recs) and int(recs["name_off"][i]) == name_off, (site, name)
            assert int(recs["name_len"][i]) == len(name) and text[name_off:name_off + len(name)] == name, (site, name)
            if seq_len is not None:
                assert int(recs["seq_len"][i]) == seq_len and int(recs["n_valid_kmers"][i]) == max(0, seq_len - k + 1), (site, name)
        if p["crossing"]:                                    # the oldest window across B begins with the motif
            at = _oldest_crossing_start(text, B, p["reach"])
            assert text[at:at + len(inputs.SEAM_MOTIF)] == inputs.SEAM_MOTIF, site
        else:                                                # no window across B: the first one behind it does
            at = text.index(b"\n", B) + 1 if kind in ("header_across", "header_at", "blank_gt") else B
            assert text[at:at + len(inputs.SEAM_MOTIF)] == inputs.SEAM_MOTIF, site
        _check_kind(text, kind, d, B, k, recs)
        assert _split_differs(text, whole, k, B), f"{site}: counting text[:B] and text[B:] apart gives the count of the text"


def _check_kind(text: bytes, kind: str, d: int, B: int, k: int, recs):
    """The bytes around B are the ones the kind names."""
    def record_at(off):                                      # index of the record whose header begins at or before `off`
        return int(np.searchsorted(recs["name_off"], off + 1, side="right")) - 1

    if kind == "header_across":
        assert text[B - d] == ord(">") and text[B - d - 1] == 10 and b"\n" not in text[B - d:B + 1] and text.index(b"\n", B) > B
        if d == 20000:
            assert B - d < B - CHUNK and set(text[B - CHUNK:B]) == {ord("h")}
    elif kind == "header_at":
        assert text[B - 1] == 10 and text[B] == ord(">") and text[B - 2] in b"ACGT"
    elif kind == "header_ends":
        assert text[B - 1] == 10 and text[B] in b"ACGT" and text.rindex(b">", 0, B) > text.rindex(b"\n", 0, B - 1)
    elif kind == "crlf_split":
        assert text[B - 1:B + 1] == b"\r\n" and text[B - 63:B - 61] == b"\r\n" and text[B + 61:B + 63] == b"\r\n"
        r = record_at(B)
        assert text[int(recs["name_off"][r]):][:10] == b"crlf_lines"
    elif kind == "blank_gt":
        assert text[B - 4:B + 1] == b"\n  \t>"
    elif kind == "pending_blanks_base":
        assert text[B - d:B] == b" " * d and text[B - d - 1] in b"ACGT" and text[B] in b"ACGT"
        assert b"\n" not in text[B - d - 30:B + 40]
    elif kind == "pending_blanks_eol":
        assert text[B - d:B] == b" " * d and text[B - d - 1] in b"ACGT" and text[B] == 10 and text[B + 1] in b"ACGT"
    elif kind == "N":
        assert text[B - d - 1] == ord("N") and set(text[B - d:B + 40]) <= set(b"ACGT") and text[B - d - 2] in b"ACGT"
    elif kind == "empty_chunks":
        assert text[B - 2 * CHUNK:B] == b"\n" * (2 * CHUNK) and text[B - 2 * CHUNK - 1] in b"ACGT" and text[B] in b"ACGT"
    elif kind == "tiny_records":
        half = inputs.TINY_RECORDS // 2
        r = record_at(B)
        name = text[int(recs["name_off"][r]):][:int(recs["name_len"][r])]
        assert name == b"t%d" % (half - 1) and int(recs["seq_len"][r]) == k + 1 and int(recs["n_valid_kmers"][r]) == 2
        assert set(text[B - (k - 1):B + 2]) <= set(b"ACGT") and text[B - k] == 10 and text[B + 2] == 10
        first, last = r - (half - 1), r + half
        assert [text[int(o):int(o) + int(n)] for o, n in zip(recs["name_off"][first:last + 1], recs["name_len"][first:last + 1])] \
            == [b"t%d" % i for i in range(inputs.TINY_RECORDS)]
        assert sorted(set(recs["seq_len"][first:last + 1].tolist())) == list(range(k + 2))
        assert B - 4000 <= int(recs["name_off"][first]) and int(recs["name_off"][last]) <= B + 4000
    else:
        raise KeyError(kind)


def test_every_kind_is_in_a_case():
    for k in (11, 15):
        kinds = inputs.tile_site_kinds(k)
        assert len(kinds) == len(set(kinds)) == 22
        cases = inputs.tile_cases(k)
        assert all(1 <= len(c) <= 4 for c in cases) and sorted((kind, d) for c in cases for kind, d, _ in c) == sorted(kinds)
        assert all(B % TILE == 0 and 0 < B <= 4 * TILE for c in cases for _, _, B in c)
        second = inputs.tile_second_feed_cases(k)
        assert sorted((kind, d) for c in second for kind, d, _ in c) == sorted(kinds)
        assert {kind for c in second for kind, _, B in c if B > inputs.TILE_FEEDS[0]} == {kind for kind, _ in kinds}
        for c in second:                                     # one site on each feed's own tile seam
            assert [B for _, _, B in c] == [TILE, inputs.TILE_FEEDS[0] + TILE]
        assert all(n > TILE and -(-n // CHUNK) > 1024 for n in inputs.TILE_FEEDS)


@pytest.mark.parametrize("case", range(6))
@pytest.mark.parametrize("k", [11, 15])
def test_tile_seam_sites(k, case):
    """The single-feed cases of test_indexer_tile_seams."""
    sites_at = inputs.tile_cases(k)[case]
    plan = {}
    text, sites = inputs.tile_seam_fasta(k, sites_at, seed=1000 * k + case, plan=plan)
    assert sorted(sites) == sorted(sites_at) and len(text) < 5 * TILE
    _check_sites(text, sites, plan, k)


@pytest.mark.parametrize("case", range(11))
def test_tile_seam_sites_of_the_second_feed(case):
    k = 11
    sites_at = inputs.tile_second_feed_cases(k)[case]
    plan = {}
    text, sites = inputs.tile_seam_fasta(k, sites_at, seed=2000 * k + case, plan=plan, n_bytes=sum(inputs.TILE_FEEDS), gap_chunks=2)
    assert len(text) == sum(inputs.TILE_FEEDS)
    assert all(hi <= inputs.TILE_FEEDS[0] or lo >= inputs.TILE_FEEDS[0] for lo, hi in (p["span"] for p in plan.values()))
    _check_sites(text, sites, plan, k, gap_chunks=2)


@pytest.mark.parametrize("site", range(3))
@pytest.mark.parametrize("k", [19, 21])
def test_deep_tile_seam_sites(k, site):
    plan = {}
    text, sites = inputs.tile_seam_fasta(k, [inputs.tile_deep_sites(k)[site]], seed=3000 + 10 * k + site, plan=plan)
    assert len(sites) == 1 and sites[0][2] == TILE
    _check_sites(text, sites, plan, k)


def test_query_tile_seam_sites():
    k = 9
    plan = {}
    text, sites = inputs.tile_seam_fasta(k, inputs.tile_query_sites(k), seed=4009, plan=plan, n_bytes=inputs.QUERY_TILE_BYTES, gap_chunks=1)
    assert len(text) == inputs.QUERY_TILE_BYTES and -(-len(text) // CHUNK) == 2 * 1024 + 5
    cut = inputs.QUERY_TILE_CUT
    assert cut > TILE and len(text) - cut > TILE
    assert {B for _, _, B in sites} == {TILE, 2 * TILE, cut + TILE}
    _check_sites(text, sites, plan, k, gap_chunks=1)
    recs = oracle.kmer_list(text, k, records=True)[1]["records"]
    assert int(recs["name_off"][0]) == 1 and int(recs["name_off"][1]) > TILE, "the first record runs on across chunk 1024"


@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("n_chunks", [1025, 2049, 3 * 1024 + 1])
def test_fastq_scan_run_seams(n_chunks, crlf):
    fq, fa, names_at, placed = fastq_ref.seam_read_set(n_chunks, crlf, seed=n_chunks + crlf)
    per = -(-n_chunks // fastq_ref.SCAN_RUNS)
    assert per == {1025: 2, 2049: 3, 3073: 4}[n_chunks] and -(-len(fq) // CHUNK) == n_chunks
    n_runs = -(-n_chunks // per)
    assert n_runs == {1025: 513, 2049: 683, 3073: 769}[n_chunks]
    run = per * CHUNK
    if n_chunks == 1025:                                     # the builder is the same at every size
        assert fastq_ref.fastq_to_fasta(fq) == fa
        assert fastq_ref.stats(fq) == {"records": len(names_at), "lines": 4 * len(names_at), "bytes_fed": len(fq), "bytes_emitted": len(fa)}
        assert all(fq[int(a):].startswith(fa[int(o):int(o) + 8]) for a, o in zip(names_at[::997], oracle.kmer_list(fa, 11, records=True)[1]["records"]["name_off"][::997]))
    seams = np.arange(1, n_runs, dtype=np.int64) * run
    assert set(placed.values()) <= set(seams.tolist()) and len(set(placed.values())) == 5
    buf = np.frombuffer(fq, dtype=np.uint8)
    line_of = np.concatenate([[0], np.cumsum(buf == 10)])[seams]          # terminators in front of the seam: the line it lies in
    roles = np.bincount(line_of % 4, minlength=4)
    assert (roles >= 1).all() and roles[[1, 3]].min() >= 100, roles
    B = placed["crlf"]
    assert fq[B - 1:B + 1] == b"\r\n" and line_of[B // run - 1] % 4 == 1
    B = placed["at_quality"]
    assert fq[B - 1:B + 1] == b"\n@" and line_of[B // run - 1] % 4 == 3
    B = placed["plus_line"]
    assert fq[B - 1:B + 1] == b"\n+" and line_of[B // run - 1] % 4 == 2
    B = placed["empty_read"]
    assert fq[B - 1] == 10 and fq[B] in b"\r\n" and line_of[B // run - 1] % 4 == 1
    assert b">placed_empty" + (b"\r\n\r\n" if crlf else b"\n\n") in fa
    B = placed["name_across"]
    assert fq[B - 6:B - 4] == b"\n@" and line_of[B // run - 1] % 4 == 0 and fq.index(b"\n", B) > B + 10
    assert (fq.count(b"\r\n") == fq.count(b"\n")) == crlf and fq.count(b"\r\n") >= 4
