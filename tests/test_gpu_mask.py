"""GPU: the masked text (kmer_cover.hip k_mask_apply, pk_query_set_mask / pk_query_mask_text / pk_query_mask_counts,
pykmer_amd.mask) and mask.py end to end, against the host restatement mask_ref: every output byte for byte, every count
exactly."""
import gzip
import json
import os

import numpy as np
import pytest

import gpu_support as gs
import byte_inputs
import mask_inputs as mi
import mask_ref
import query_coords_inputs as qci
import query_ref
from gpu_support import lib, run_py

pytestmark = pytest.mark.gpu
CHUNK = mi.CHUNK
MODES = ((False, False), (True, False), (False, True), (True, True))          # (hard, invert)


def _apply(text: bytes, bits, n_bases: int, hard=False, invert=False, cuts=None, q=None):
    """The text through one applying indexer, fed in the pieces `cuts` make: (masked text, masked (R,), bases seen)."""
    lib = gs.lib()
    own = q is None
    q = lib.QueryIndexer(1, device=0) if own else q
    try:
        q.set_mask(bits, n_bases, hard=hard, invert=invert)
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
        assert q.timings()["mask_s"] > 0 or not text
        return b"".join(out), masked.copy(), seen
    finally:
        if own:
            q.close()


def _check(text, want, got, hard, invert, cover=None):
    out, masked, seen = got
    ref = mask_ref.masked_text(text, want, hard, invert, cover)
    assert len(out) == len(text) and seen == want["n_bases"]
    if out != ref:
        a, b = np.frombuffer(out, dtype=np.uint8), np.frombuffer(ref, dtype=np.uint8)
        raise AssertionError(f"masked text differs at bytes {np.flatnonzero(a != b)[:8]}")
    assert masked.dtype == np.uint64 and np.array_equal(masked, mask_ref.masked_counts(want, invert, cover))


@pytest.mark.parametrize("name", [n for n, _ in mi.texts(9)])
def test_masked_text_of_every_text(gpu, name):
    k = 9
    text = dict(mi.texts(k))[name]
    want = mask_ref.expected(text, k, mi.band_tables(k), 2, 254)
    for hard, invert in MODES:
        _check(text, want, _apply(text, want["bits"], want["n_bases"], hard, invert), hard, invert)
    cuts = sorted({c for c in (7, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 4096 + 33, len(text) - 1) if c < len(text)})
    assert len(cuts) >= 5
    _check(text, want, _apply(text, want["bits"], want["n_bases"], True, True, cuts), True, True)
    soft = _apply(text, want["bits"], want["n_bases"])[0]
    assert soft.upper() == text.upper()


def _byte_texts():
    extra = (b"acgtACGTNN dead\r\n\r>r1 x\r\nACGTacgtNNacgtTTGACCA\rGGTCAttgacc  A\r\n\n>r2\nacgtacgtacgtTTGACCATGACGTA\r\n>r3\r\rTTGACGGTCATTGGTCA" * 40
             + b"\n>last\nACGTTGCAAGGTCATTGACC")                 # lower case, CRLF, lone CR, dead text, no final newline
    return [("soup_31", byte_inputs.soup(31, 69_999)), ("soup_35", byte_inputs.soup(35, 16_385)), ("line_starts", byte_inputs.line_start_fasta()),
            ("headers", byte_inputs.header_bytes_fasta()), ("blanks", qci.blanks()), ("crlf", extra)]


@pytest.mark.parametrize("name", [n for n, _ in _byte_texts()])
def test_all_byte_values_outside_and_inside_sequence_lines(gpu, name):
    k = 5
    text = dict(_byte_texts())[name]
    tables = query_ref.random_tables(k, 1, seed=1910)
    want = mask_ref.expected(text, k, tables, 255, 255)
    assert 0 < want["cover"].sum() < want["n_bases"]
    for hard, invert in MODES:
        _check(text, want, _apply(text, want["bits"], want["n_bases"], hard, invert), hard, invert)
    if name.startswith("soup"):
        cuts = byte_inputs.cuts_around_odd_bytes(text, seed=1911)
        _check(text, want, _apply(text, want["bits"], want["n_bases"], True, False, sorted(set(int(c) for c in cuts))), True, False)
    if name == "crlf":
        assert not text.endswith(b"\n") and b"\r>" in text and want["valid"][:8].sum() == 0


def test_feeds_cut_anywhere(gpu):
    """The text cut at every offset around a chunk seam and inside a header; short reads behind a small first feed (the
    second feed's squeeze backs out and the feed runs again: masked[] must not count twice); one indexer, reset between."""
    k = mi.SEAM_K
    text = mi.seam_text()
    want = mask_ref.expected(text, k, [mi.seam_tables()[0]], 1, 255)
    with lib().QueryIndexer(1, device=0) as q:
        for cut in list(range(CHUNK - 11, CHUNK + 12)) + [1, 3, text.index(b"\n"), text.index(b"\n") + 1]:
            _check(text, want, _apply(text, want["bits"], want["n_bases"], True, False, [cut], q=q), True, False)
            q.reset()
        _check(text, want, _apply(text, want["bits"], want["n_bases"], False, True, mi.line_cuts(), q=q), False, True)
    reads = qci.short_reads()
    rw = mask_ref.expected(reads, 5, mi.band_tables(5), 1, 255)
    assert rw["n_records"] == 5000 > 4096
    for hard, invert in ((False, False), (True, True)):
        _check(reads, rw, _apply(reads, rw["bits"], rw["n_bases"], hard, invert, [200]), hard, invert)
    long_text, table = mi.long_text()                       # more chunks than the scan tile, in one feed
    lw = mask_ref.expected(long_text, k, [table], 1, 255, fast=True)
    _check(long_text, lw, _apply(long_text, lw["bits"], lw["n_bases"], True, False), True, False)


def test_bits_of_the_wrong_length_and_all_ones(gpu):
    lib = gs.lib()
    text = qci.blanks()
    want = mask_ref.expected(text, 5, mi.band_tables(5), 1, 255)
    n = want["n_bases"]
    ones = np.full((n + 7) // 8, 0xFF, dtype=np.uint8)
    every = np.ones(n, dtype=bool)
    got = _apply(text, ones, n)
    _check(text, want, got, False, False, cover=every)
    a, b = np.frombuffer(got[0], dtype=np.uint8), np.frombuffer(text, dtype=np.uint8)
    changed = np.flatnonzero(a != b)
    assert np.array_equal(changed, np.flatnonzero(want["valid"] & (b < 0x60))) and int(got[1].sum()) == n
    _check(text, want, _apply(text, ones, n, hard=True, invert=True), True, True, cover=every)       # nothing is selected
    with lib.QueryIndexer(1, device=0) as q:
        with pytest.raises(ValueError, match="bytes of cover bits"):
            q.set_mask(ones[:-1], n)
        with pytest.raises(ValueError, match="bytes of cover bits"):
            q.set_mask(np.concatenate([ones, ones]), n)
    for wrong in (n - 9, n + 1000, 0):                        # bits for another stream: an error return, and no fault
        with pytest.raises(lib.PkError) as exc:
            _apply(text, np.full((wrong + 7) // 8, 0xFF, dtype=np.uint8), wrong)
        assert exc.value.code == lib.PK_ERR_STATE and "changed between the phases" in str(exc.value)


@pytest.fixture(scope="module")
def kins(gpu, tmp_path_factory):
    """([donor.kin, host.kin], [donor table, host table]) at k = 5, written here by indexer.py."""
    import oracle
    d = tmp_path_factory.mktemp("mask_tables")
    paths, tabs = [], []
    for name, seq in (("donor", mi.DONOR), ("host", mi.HOST)):
        fa, data = d / f"{name}.fa", b">" + name.encode() + b"\n" + seq + b"\n"
        fa.write_bytes(data)
        run_py("indexer.py", str(fa), name, "5", cwd=str(d))
        paths.append(f"{fa}.05.kin")
        tabs.append(oracle.count_fasta(data, 5)["table"])
    return paths, tabs


def test_both_phases_through_files(gpu, kins, tmp_path):
    """mask.mask_records on a plain and a gzip file: cover bits, masked text and counts; apply_mask with bits from elsewhere."""
    from pykmer_amd import mask
    paths, tabs = kins
    text = mi.TOOL_FASTA
    want = mask_ref.expected(text, 5, tabs, 1, 255)
    assert 0 < want["cover"].sum() < want["n_bases"]
    plain = tmp_path / "in.fa"
    plain.write_bytes(text)
    gz = tmp_path / "in2.fa.gz"
    with gzip.open(gz, "wb") as fh:
        fh.write(text)
    for n, (src, (hard, invert)) in enumerate(zip((plain, gz, plain, gz), MODES)):
        res = mask.mask_records(str(src), paths, 1, 255, hard=hard, invert=invert, project_name=str(tmp_path / f"p{n}"), hbm_budget=1 << 40)
        assert res["n_bases"] == want["n_bases"] and np.array_equal(res["cover"], want["bits"]) and res["n_groups"] == 1
        assert open(res["output"], "rb").read() == mask_ref.masked_text(text, want, hard, invert)
        assert np.array_equal(res["masked"], mask_ref.masked_counts(want, invert)) and res["bytes"] == len(text)
    two = mask.cover_bits(str(plain), paths, 1, 255, hbm_budget=4 ** 5 + 100)
    assert two["n_groups"] == 2 and np.array_equal(two["cover"], want["bits"])
    other = mask_ref.pack(np.arange(want["n_bases"]) % 3 == 0)
    done = mask.apply_mask(str(gz), other, want["n_bases"], tmp_path / "o.fa", hard=True)
    assert (tmp_path / "o.fa").read_bytes() == mask_ref.masked_text(text, want, True, False, cover=mask_ref.unpack(other, want["n_bases"]))
    assert done["n_masked"] == int(mask_ref.unpack(other, want["n_bases"]).sum()) and done["mask_s"] > 0
    with pytest.raises(ValueError, match="changed between the phases"):
        mask.apply_mask(str(plain), other[:-1], want["n_bases"] - 8, tmp_path / "never.fa")
    assert not (tmp_path / "never.fa").exists()


@pytest.mark.parametrize("form", ["plain", "gz"])
def test_cli(gpu, kins, tmp_path, form):
    paths, tabs = kins
    text = mi.TOOL_FASTA
    src = tmp_path / ("q.fa" if form == "plain" else "q.fa.gz")
    if form == "plain":
        src.write_bytes(text)
    else:
        with gzip.open(src, "wb") as fh:
            fh.write(text)
    proj = str(tmp_path / "cli")
    argv = ["mask.py", proj, str(src)] + paths + ["--min-count", "1", "--max-count", "254", "--hard"]
    r = run_py(*argv, cwd=str(tmp_path))
    want = mask_ref.expected(text, 5, tabs, 1, 254)
    assert 0 < want["cover"].sum() < want["n_bases"]
    assert open(proj + ".masked.fa", "rb").read() == mask_ref.masked_text(text, want, True, False)
    z = np.load(proj + ".kmm")
    assert set(z.files) == {"masked", "n_valid", "seq_len", "kmer_len", "min_count", "max_count", "hard", "invert", "n_bases"}
    assert np.array_equal(z["masked"], mask_ref.masked_counts(want)) and int(z["n_bases"]) == want["n_bases"] and bool(z["hard"]) and not bool(z["invert"])
    assert int(z["kmer_len"]) == 5 and int(z["max_count"]) == 254 and z["masked"].dtype == np.uint64
    meta = json.load(open(proj + ".kmm.json"))
    for key in ("project_name", "kmer_len", "min_count", "max_count", "query_file", "records", "data", "mode", "invert", "n_records", "n_bases",
                "n_masked", "bytes", "output", "lookup_s", "mask_s"):
        assert key in meta, key
    assert meta["mode"] == "hard" and meta["n_masked"] == int(want["cover"].sum()) and meta["bytes"] == len(text) and meta["output"] == proj + ".masked.fa"
    assert meta["n_records"] == want["n_records"] == len(meta["records"]) and meta["records"][0] == "donor piece"
    last = r.stdout.strip().split("\n")[-1]
    assert last == f"{int(want['cover'].sum())} of {want['n_bases']} valid bases masked in {want['n_records']} records, {proj}.masked.fa"
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]
    again = run_py(*argv, cwd=str(tmp_path), status=1)
    assert [ln for ln in again.stderr.split("\n") if ln.startswith("error: ") and "already exists" in ln]
