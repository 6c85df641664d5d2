"""GPU: the masked intervals (kmer_intervals.hip, pk_query_set_intervals / pk_query_intervals, pykmer_amd.mask) and
mask.py --bed end to end, against the host restatement mask_bed_ref: equal uint64 arrays.  In every case the masked text and
masked[] are still what mask_ref says: the intervals must not disturb the apply."""
import gzip
import json
import os

import numpy as np
import pytest

import gpu_support as gs
import byte_inputs
import mask_bed_ref
import mask_inputs as mi
import mask_ref
import query_coords_inputs as qci
import query_ref
from gpu_support import lib, run_py

pytestmark = pytest.mark.gpu
CHUNK = mi.CHUNK
MODES = ((False, False), (True, False), (False, True), (True, True))          # (hard, invert)
# the `crlf` text of test_gpu_mask.py: lower case, CRLF, lone CR, dead text, no final newline
CRLF = (b"acgtACGTNN dead\r\n\r>r1 x\r\nACGTacgtNNacgtTTGACCA\rGGTCAttgacc  A\r\n\n>r2\nacgtacgtacgtTTGACCATGACGTA\r\n>r3\r\rTTGACGGTCATTGGTCA" * 40
        + b"\n>last\nACGTTGCAAGGTCATTGACC")
ANY_TABLE = [np.ones(4, dtype=np.uint8)]                     # k = 1: for texts of which only the valid bases matter


def _apply(text: bytes, bits, n_bases: int, hard=False, invert=False, cuts=None, q=None, intervals=True):
    """The text through one applying indexer with the intervals on, fed in the pieces `cuts` make: (masked text, masked (R,),
    bases seen, (iv_record, iv_start, iv_end))."""
    lib = gs.lib()
    own = q is None
    q = lib.QueryIndexer(1, device=0) if own else q
    try:
        q.set_mask(bits, n_bases, hard=hard, invert=invert)
        if intervals:
            q.set_intervals(True)
        buf, out, pos = np.frombuffer(text, dtype=np.uint8), [], 0
        room = np.empty(len(text) + 1, dtype=np.uint8)
        for c in list(cuts or []) + [len(text)]:
            if c > pos:
                q.feed(buf[pos:c])
                got = q.mask_text(room)
                assert got.size == c - pos
                out.append(got.tobytes())
                pos = c
        fin = q.finish()
        masked, seen = q.mask_counts(fin["n_records"])
        iv = tuple(a.copy() for a in q.intervals()) if intervals else None
        assert not intervals or q.interval_seconds() > 0 or not text
        return b"".join(out), masked.copy(), seen, iv
    finally:
        if own:
            q.close()


def _same_intervals(got, ref):
    for name, a, b in zip(("iv_record", "iv_start", "iv_end"), got, ref):
        assert a.dtype == np.uint64 and a.shape == b.shape, (name, a.dtype, a.shape, b.shape)
        if not np.array_equal(a, b):
            at = np.flatnonzero(a != b)[:5]
            raise AssertionError(f"{name} differs at rows {at}: got {a[at]}, want {b[at]}")


def _check(text, want, got, hard, invert, ref, cover=None):
    out, masked, seen, iv = got
    assert len(out) == len(text) and seen == want["n_bases"]
    if out != mask_ref.masked_text(text, want, hard, invert, cover):
        raise AssertionError("the masked text differs with the intervals on")
    assert masked.dtype == np.uint64 and np.array_equal(masked, mask_ref.masked_counts(want, invert, cover))
    _same_intervals(iv, ref)


def _refs(text, want, cover=None):
    """The reference intervals of both selections: {invert: (iv_record, iv_start, iv_end)}."""
    return {inv: mask_bed_ref.intervals(text, mask_bed_ref.selected_bytes(text, want, inv, cover)) for inv in (False, True)}


@pytest.mark.parametrize("name", [n for n, _ in mi.texts(9)])
def test_intervals_of_every_text(gpu, name):
    k = 9
    text = dict(mi.texts(k))[name]
    want = mask_ref.expected(text, k, mi.band_tables(k), 2, 254)
    refs = _refs(text, want)
    assert refs[False][0].size > 1 and refs[True][0].size > 1
    for hard, invert in MODES:
        _check(text, want, _apply(text, want["bits"], want["n_bases"], hard, invert), hard, invert, refs[invert])
    cuts = sorted({c for c in (7, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 4096 + 33, len(text) - 1) if c < len(text)})
    assert len(cuts) >= 5
    for hard, invert in ((True, True), (False, False)):
        _check(text, want, _apply(text, want["bits"], want["n_bases"], hard, invert, cuts), hard, invert, refs[invert])


@pytest.mark.parametrize("name", ["blanks", "crlf"])
def test_structure_without_tables(gpu, name):
    """All-ones bits: the intervals are the maximal runs of valid bases -- interior and trailing blanks, CRLF, lone CR, dead text
    before the first header, N, no final newline."""
    text = {"blanks": qci.blanks(), "crlf": CRLF}[name]
    want = mask_ref.expected(text, 1, ANY_TABLE)
    n = want["n_bases"]
    ones, every = np.full((n + 7) // 8, 0xFF, dtype=np.uint8), np.ones(n, dtype=bool)
    refs = _refs(text, want, every)
    assert refs[False][0].size > want["n_records"] // 2 and int((refs[False][2] - refs[False][1]).sum()) == n
    _check(text, want, _apply(text, ones, n), False, False, refs[False], cover=every)
    cuts = sorted({c for c in (5, 63, 64, 65, 1000, CHUNK, len(text) - 2) if c < len(text)})
    _check(text, want, _apply(text, ones, n, True, False, cuts), True, False, refs[False], cover=every)
    got = _apply(text, ones, n, False, True)                 # nothing is selected
    _check(text, want, got, False, True, refs[True], cover=every)
    assert all(a.shape == (0,) and a.dtype == np.uint64 for a in got[3])
    if name == "crlf":
        assert not text.endswith(b"\n") and b"\r>" in text and want["valid"][:8].sum() == 0


def test_capacity_and_growth(gpu):
    """One interval per selected base, 20 000 of them in three chunks: the rows outgrow their first capacity."""
    text = mi.seam_text()
    want = mask_ref.expected(text, 1, ANY_TABLE)
    n = want["n_bases"]
    assert n == 40_000
    for cover, length, count in ((np.arange(n) % 2 == 0, 1, 20_000), (np.arange(n) % 3 != 0, 2, 13_333)):
        ref = mask_bed_ref.intervals(text, mask_bed_ref.selected_bytes(text, want, False, cover))
        assert ref[0].size == count and ((ref[2] - ref[1]) == length).all()
        _check(text, want, _apply(text, mask_ref.pack(cover), n), False, False, ref, cover=cover)
        _check(text, want, _apply(text, mask_ref.pack(cover), n, True, False, [CHUNK - 3, CHUNK + 1, 2 * CHUNK]), True, False, ref, cover=cover)


def test_seams_and_feeds_cut_anywhere(gpu):
    """A run that is open at a cut comes out as one interval: every offset around a chunk seam, inside the header, one byte
    at a time over a line; one indexer, reset between."""
    k = mi.SEAM_K
    text = mi.seam_text()
    want = mask_ref.expected(text, k, [mi.seam_tables()[0]], 1, 255)
    refs = _refs(text, want)
    off = want["base_off"]
    first = int(np.searchsorted(off, CHUNK))
    assert want["cover"][first - 1] and want["cover"][first]                             # a run lies across the seam
    with lib().QueryIndexer(1, device=0) as q:
        for cut in list(range(CHUNK - 11, CHUNK + 12)) + [1, 3, text.index(b"\n"), text.index(b"\n") + 1]:
            _check(text, want, _apply(text, want["bits"], want["n_bases"], True, False, [cut], q=q), True, False, refs[False])
            q.reset()
        _check(text, want, _apply(text, want["bits"], want["n_bases"], False, True, mi.line_cuts(), q=q), False, True, refs[True])
        q.reset()
        _check(text, want, _apply(text, want["bits"], want["n_bases"], False, False, mi.line_cuts(), q=q), False, False, refs[False])


def _blank_seam(boundary: int, follows: bytes) -> bytes:
    """One record whose first `boundary` bytes end in three blanks inside a sequence line; `follows` comes next."""
    head = b">r\n"
    fill = (b"ACGGTCATTGACCA" * (boundary // 14 + 1))[:boundary - len(head) - 3]
    return head + fill + b" \t " + follows + b"GATTACA\n>s\nAC GT\n"


@pytest.mark.parametrize("boundary,cut", [(40, True), (64, False), (64, True), (CHUNK, False), (CHUNK, True)])
def test_a_blank_across_a_seam(gpu, boundary, cut):
    """Blanks at the end of a feed, a piece or a chunk: interior if a base follows on the line (the run breaks and the blanks
    hold positions), trailing if a terminator follows (the run goes on across the line)."""
    for follows, runs_in_r in ((b"T", 2), (b"\nT", 1), (b"\r\n\n \nT", 1)):
        text = _blank_seam(boundary, follows)
        assert text[boundary - 3:boundary] == b" \t " and text[boundary:boundary + 1] == follows[:1]
        want = mask_ref.expected(text, 1, ANY_TABLE)
        n = want["n_bases"]
        every = np.ones(n, dtype=bool)
        ref = mask_bed_ref.intervals(text, mask_bed_ref.selected_bytes(text, want, False, every))
        assert int((ref[0] == 0).sum()) == runs_in_r and ref[0].size == runs_in_r + 2
        if runs_in_r == 2:
            assert int(ref[1][1]) == int(ref[2][0]) + 3      # the three blanks hold positions
        got = _apply(text, np.full((n + 7) // 8, 0xFF, dtype=np.uint8), n, cuts=[boundary] if cut else None)
        _check(text, want, got, False, False, ref, cover=every)


def test_a_run_across_a_hollow_chunk(gpu):
    text, table = mi.hollow()
    want = mask_ref.expected(text, mi.SEAM_K, [table], 1, 255)
    refs = _refs(text, want)
    rec, pos = mask_bed_ref.positions(text)
    across = [(a, b) for a, b in zip(refs[False][1], refs[False][2]) if a <= pos[CHUNK - 2] and b > pos[2 * CHUNK + 1]]
    assert len(across) == 1                                  # one run from the first chunk through the three bases into the third
    for invert in (False, True):
        _check(text, want, _apply(text, want["bits"], want["n_bases"], False, invert), False, invert, refs[invert])
    _check(text, want, _apply(text, want["bits"], want["n_bases"], True, False, [CHUNK + 5, 2 * CHUNK - 1]), True, False, refs[False])


def test_short_reads_behind_a_small_first_feed(gpu):
    """5000 records behind a 200-byte first feed: the squeeze backs out and the feed runs again; no interval doubled or lost."""
    reads = qci.short_reads()
    want = mask_ref.expected(reads, 5, mi.band_tables(5), 1, 255)
    assert want["n_records"] == 5000 > 4096
    refs = _refs(reads, want)
    rec, pos = mask_bed_ref.positions(reads)
    seq_len = np.bincount(rec[pos >= 0], minlength=5000)
    at_end = refs[True][2] == seq_len[refs[True][0].astype(np.int64)].astype(np.uint64)
    assert at_end[:-1].sum() > 100 and at_end[-1] and int(refs[True][0][-1]) == 4999   # runs that end at a header and at the end of the stream
    for hard, invert in ((False, False), (True, True)):
        _check(reads, want, _apply(reads, want["bits"], want["n_bases"], hard, invert, [200]), hard, invert, refs[invert])


def test_more_chunks_than_the_scan_tile(gpu):
    text, table = mi.long_text()
    want = mask_ref.expected(text, mi.SEAM_K, [table], 1, 255, fast=True)
    ref = mask_bed_ref.intervals_one_plain_record(text, want, want["cover"])
    assert 1 < ref[0].size < 1000
    _check(text, want, _apply(text, want["bits"], want["n_bases"], True, False), True, False, ref)
    inv = mask_bed_ref.intervals_one_plain_record(text, want, ~want["cover"])
    assert int(inv[2][-1] - inv[1][0]) > 1025 * CHUNK * 60 // 61 - 1000                 # runs open across the tile seam
    _check(text, want, _apply(text, want["bits"], want["n_bases"], False, True), False, True, inv)


@pytest.mark.parametrize("seed,size", [(31, 69_999), (35, 16_385)])
def test_soups_of_all_byte_values(gpu, seed, size):
    k = 5
    text = byte_inputs.soup(seed, size)
    want = mask_ref.expected(text, k, query_ref.random_tables(k, 1, seed=1910), 255, 255)
    assert 0 < want["cover"].sum() < want["n_bases"]
    refs = _refs(text, want)
    for hard, invert in MODES:
        _check(text, want, _apply(text, want["bits"], want["n_bases"], hard, invert), hard, invert, refs[invert])
    cuts = sorted(set(int(c) for c in byte_inputs.cuts_around_odd_bytes(text, seed=1911)))
    for invert in (False, True):
        _check(text, want, _apply(text, want["bits"], want["n_bases"], True, invert, cuts), True, invert, refs[invert])


def test_errors(gpu):
    lib = gs.lib()
    text = qci.blanks()
    want = mask_ref.expected(text, 1, ANY_TABLE)
    n = want["n_bases"]
    ones = np.full((n + 7) // 8, 0xFF, dtype=np.uint8)
    with lib.QueryIndexer(1, device=0) as q:
        with pytest.raises(ValueError, match="bytes of cover bits"):
            q.set_mask(ones[:-1], n)
        with pytest.raises(lib.PkError) as exc:              # no mask yet
            q.set_intervals(True)
        assert exc.value.code == lib.PK_ERR_STATE
        q.set_mask(ones, n)
        gs.feed(q, text)
        with pytest.raises(lib.PkError) as exc:              # after a feed
            q.set_intervals(True)
        assert exc.value.code == lib.PK_ERR_STATE
        q.finish()
        with pytest.raises(lib.PkError) as exc:              # the intervals are off
            q.intervals()
        assert exc.value.code == lib.PK_ERR_STATE
        q.reset()
        q.set_mask(ones, n)
        q.set_intervals(True)
        q.reset()                                            # a reset clears the setting
        q.set_mask(ones, n)
        gs.feed(q, text)
        q.finish()
        with pytest.raises(lib.PkError) as exc:
            q.interval_seconds()
        assert exc.value.code == lib.PK_ERR_STATE
    for wrong in (n - 9, n + 1000, 0):                        # bits for another stream: the error returns of today, and no intervals
        with pytest.raises(lib.PkError) as exc:
            _apply(text, np.full((wrong + 7) // 8, 0xFF, dtype=np.uint8), wrong)
        assert exc.value.code == lib.PK_ERR_STATE and "changed between the phases" in str(exc.value)
        with lib.QueryIndexer(1, device=0) as q:
            q.set_mask(np.full((wrong + 7) // 8, 0xFF, dtype=np.uint8), wrong)
            q.set_intervals(True)
            gs.feed(q, text)
            q.finish()
            with pytest.raises(lib.PkError) as exc:
                q.intervals()
            assert exc.value.code == lib.PK_ERR_STATE and "changed between the phases" in str(exc.value)


@pytest.fixture(scope="module")
def kins(gpu, tmp_path_factory):
    """([donor.kin, host.kin], [donor table, host table]) at k = 5, written here by indexer.py (as in test_gpu_mask.py)."""
    import oracle
    d = tmp_path_factory.mktemp("mask_bed_tables")
    paths, tabs = [], []
    for name, seq in (("donor", mi.DONOR), ("host", mi.HOST)):
        fa, data = d / f"{name}.fa", b">" + name.encode() + b"\n" + seq + b"\n"
        fa.write_bytes(data)
        run_py("indexer.py", str(fa), name, "5", cwd=str(d))
        paths.append(f"{fa}.05.kin")
        tabs.append(oracle.count_fasta(data, 5)["table"])
    return paths, tabs


KMM_KEYS = {"masked", "n_valid", "seq_len", "kmer_len", "min_count", "max_count", "hard", "invert", "n_bases"}
JSON_KEYS = {"project_name", "kmer_len", "min_count", "max_count", "query_file", "records", "data", "mode", "invert", "n_records", "n_bases", "n_masked",
             "bytes", "output", "lookup_s", "mask_s"}
CHROMS = ["donor", "none", "empty", "tiny", "host", "mixed", "other", "last"]


@pytest.mark.parametrize("form", ["plain", "gz"])
def test_cli_with_bed(gpu, kins, tmp_path, form):
    paths, tabs = kins
    text = mi.TOOL_FASTA
    src = tmp_path / ("q.fa" if form == "plain" else "q.fa.gz")
    if form == "plain":
        src.write_bytes(text)
    else:
        with gzip.open(src, "wb") as fh:
            fh.write(text)
    proj = str(tmp_path / "cli")
    argv = ["mask.py", proj, str(src)] + paths + ["--min-count", "1", "--max-count", "254", "--bed"]
    r = run_py(*argv, cwd=str(tmp_path))
    want = mask_ref.expected(text, 5, tabs, 1, 254)
    ref = mask_bed_ref.intervals(text, mask_bed_ref.selected_bytes(text, want))
    assert open(proj + ".masked.fa", "rb").read() == mask_ref.masked_text(text, want, False, False)
    bed = open(proj + ".masked.bed", "rb").read()
    assert bed == mask_bed_ref.bed_lines(CHROMS, *ref) and bed.startswith(b"donor\t0\t41\n")
    z = np.load(proj + ".kmm")
    assert set(z.files) == KMM_KEYS | {"iv_record", "iv_start", "iv_end"}
    _same_intervals((z["iv_record"], z["iv_start"], z["iv_end"]), ref)
    assert np.array_equal(z["masked"], mask_ref.masked_counts(want))
    meta = json.load(open(proj + ".kmm.json"))
    assert set(meta) == JSON_KEYS | {"bed", "n_intervals", "intervals_s"}
    assert meta["bed"] == proj + ".masked.bed" and meta["n_intervals"] == ref[0].size and meta["intervals_s"] > 0
    last = r.stdout.strip().split("\n")[-1]
    assert last == (f"{int(want['cover'].sum())} of {want['n_bases']} valid bases masked in {want['n_records']} records, {proj}.masked.fa, "
                    f"{ref[0].size} intervals in {proj}.masked.bed")
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]
    again = run_py(*argv, cwd=str(tmp_path), status=1)
    assert [ln for ln in again.stderr.split("\n") if ln.startswith("error: ") and "already exists" in ln]
    if form == "plain":                                      # without --bed: exactly the former files, keys and last line
        proj2 = str(tmp_path / "old")
        r2 = run_py("mask.py", proj2, str(src), *paths, "--max-count", "254", cwd=str(tmp_path))
        assert sorted(f for f in os.listdir(tmp_path) if f.startswith("old.")) == ["old.kmm", "old.kmm.json", "old.masked.fa"]
        assert set(np.load(proj2 + ".kmm").files) == KMM_KEYS and set(json.load(open(proj2 + ".kmm.json"))) == JSON_KEYS
        assert r2.stdout.strip().split("\n")[-1] == (f"{int(want['cover'].sum())} of {want['n_bases']} valid bases masked in {want['n_records']} records, "
                                                     f"{proj2}.masked.fa")


def test_apply_mask_with_intervals_and_bits_from_elsewhere(gpu, tmp_path):
    from pykmer_amd import mask
    text = mi.TOOL_FASTA
    want = mask_ref.expected(text, 1, ANY_TABLE)
    n = want["n_bases"]
    gz = tmp_path / "in.fa.gz"
    with gzip.open(gz, "wb") as fh:
        fh.write(text)
    cover = np.arange(n) % 7 < 4
    ref = mask_bed_ref.intervals(text, mask_bed_ref.selected_bytes(text, want, False, cover))
    done = mask.apply_mask(str(gz), mask_ref.pack(cover), n, tmp_path / "o.fa", hard=True, intervals=True)
    assert (tmp_path / "o.fa").read_bytes() == mask_ref.masked_text(text, want, True, False, cover=cover)
    _same_intervals((done["iv_record"], done["iv_start"], done["iv_end"]), ref)
    assert done["n_intervals"] == ref[0].size and done["intervals_s"] > 0 and done["n_masked"] == int(cover.sum())
    plain = mask.apply_mask(str(gz), mask_ref.pack(cover), n, tmp_path / "p.fa", hard=True)
    assert "iv_record" not in plain and "n_intervals" not in plain and plain["n_masked"] == done["n_masked"]
