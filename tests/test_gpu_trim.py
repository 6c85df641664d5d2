"""GPU: the trim path -- the cover bits of FASTQ streams (pk_query_set_cover with fmt="fastq", never tested before), the
Trimmer (kmer_trim.hip, pk_trim_*) on bits from anywhere against trim_ref, the threshold, the argument errors, and trim.py
end to end as a child process.  tests/test_trim_host.py holds trim_ref against hand-worked records on the CPU."""
import ctypes
import functools
import json

import numpy as np
import pytest

import byte_inputs
import fastq_qual_ref
import fastq_ref
import gpu_support as gs
import mask_ref
import oracle
import trim_inputs
import trim_ref
from gpu_support import Device, lib, run_py, stream

pytestmark = pytest.mark.gpu
KS = (5, 7)
T = 53                                                       # the threshold byte of --min-qual 20 at offset 33


@functools.lru_cache(maxsize=None)
def _stream(k: int, final_newline: bool = True) -> bytes:
    return trim_inputs.stream(k, seed=40 + k, final_newline=final_newline)


@functools.lru_cache(maxsize=None)
def _placement_head() -> bytes:
    """The first records of byte_inputs.placement_fastq, about 60 KB: every byte value in every line role."""
    fq = byte_inputs.placement_fastq(False)
    starts = trim_ref.starts(fq)
    return fq[:int(starts[int(np.searchsorted(starts, 60_000))])]


@functools.lru_cache(maxsize=None)
def _random_case(k: int, final_newline: bool, tq: int):
    """(fq, packed bits, n_bases, the reference) for random bits over a stream: computed once, shared by the tests."""
    fq = _stream(k, final_newline)
    if tq:
        fq = fastq_qual_ref.hand_qualities(fq, tq, seed=3)
    base_rec = mask_ref.walk(trim_ref.fasta_of(fq, tq), 1)[1]
    n_valid = np.bincount(base_rec, minlength=len(trim_ref.starts(fq)) - 1)
    cover = trim_inputs.bits(n_valid, seed=50 + k)
    want = trim_ref.runs(fq, cover, T=tq)
    return fq, mask_ref.pack(cover), int(cover.size), want


def _feed_all(t, fq, starts, per):
    """The stream through a Trimmer in feeds of `per` records (None: one feed); the feeds' fields concatenated."""
    R = len(starts) - 1
    buf = np.frombuffer(fq, dtype=np.uint8)
    parts = []
    for lo in range(0, max(R, 1), per or max(R, 1)):
        hi = min(R, lo + (per or R))
        a, b = int(starts[lo]), int(starts[hi])
        parts.append(t.feed(buf[a:b], starts[lo:hi + 1] - starts[lo]))
    return {name: np.concatenate([p[name] for p in parts]) for name in lib().TRIM_FIELDS}


def _same_fields(got, want):
    for name in trim_ref.FIELDS:
        assert got[name].dtype == np.uint64 and got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape)
        assert np.array_equal(got[name], want[name]), (name, np.flatnonzero(got[name] != want[name])[:8], got[name][:8], want[name][:8])


# ------------------------------------------------------------------ layer 1: cover bits of FASTQ input
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("tq", [0, T])
def test_cover_bits_of_fastq_streams(gpu, k, tq):
    tabs = gs.tables(k, 2, seed=700 + k)
    texts = [_stream(k), _stream(k, False), _placement_head()]
    rng = np.random.default_rng(k + tq)
    with Device(tabs) as dev, lib().QueryIndexer(k, device=0, fmt="fastq", min_qual_byte=tq) as q:
        for n, fq in enumerate(texts):
            if tq:
                fq = fastq_qual_ref.hand_qualities(fq, tq, seed=n) if n % 2 == 0 else fastq_qual_ref.biased_qualities(fq, tq, 0.2, seed=n)
            fasta = trim_ref.fasta_of(fq, tq)
            for window in ((1, 255), (255, 255)):
                want = mask_ref.expected(fasta, k, tabs, *window)
                assert 0 < want["cover"].sum() < want["n_bases"]
                for cuts in (None, sorted(int(c) for c in rng.integers(1, len(fq), size=9))):
                    q.reset()
                    q.set_tables(dev.ptrs, *window)
                    got = stream(q, fq, cover=True, cuts=cuts, reset=False)
                    assert got["n_bases"] == want["n_bases"] and got["fin"]["n_records"] == want["n_records"], (n, window, cuts)
                    assert np.array_equal(got["bits"], want["bits"]), (n, window, cuts, np.flatnonzero(mask_ref.unpack(got["bits"], want["n_bases"]) != want["cover"])[:8])


# ------------------------------------------------------------------ the Trimmer on bits from anywhere
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("final_newline", [True, False])
def test_trimmer_on_random_bits(gpu, k, final_newline):
    fq, bits, n_bases, want = _random_case(k, final_newline, 0)
    starts = trim_ref.starts(fq)
    assert sorted(set(want["seq_len"].tolist())) == sorted(set(trim_inputs.lengths(k))) and fq.endswith((b"\n", b"\r")) == final_newline
    whole, cut, dropped = trim_ref.classes(want, k)
    assert min(whole, cut, dropped) >= 0.10, (whole, cut, dropped)
    length = (want["trim_end"] - want["trim_start"]).astype(np.int64)
    assert (want["covered"].astype(np.int64) > length).sum() >= 10           # reads with more than one run
    first = None
    for per in (None, 1, 7):
        with lib().Trimmer(0) as t:
            t.set_cover(bits, n_bases)
            got = _feed_all(t, fq, starts, per)
            fin = t.finish()
            timings = t.timings()
        _same_fields(got, want)
        assert fin == {"n_records": len(starts) - 1, "n_bases": n_bases, "n_covered": int(want["covered"].sum())}
        assert timings["trim_s"] > 0 and timings["feeds"] == (1 if per is None else -(-(len(starts) - 1) // per))
        first = first or got
        assert all(np.array_equal(got[name], first[name]) for name in got)


def test_device_form_and_empty_feeds(gpu):
    fq, bits, n_bases, want = _random_case(5, True, 0)
    starts = trim_ref.starts(fq)
    text = lib().DeviceBuffer(len(fq) + 1, 0)
    try:
        text.upload(np.frombuffer(b"x" + fq, dtype=np.uint8))            # the text at an odd address
        with lib().Trimmer(0) as t:
            t.set_cover(bits, n_bases)
            assert all(v.size == 0 for v in t.feed(b"", [0]).values())   # an empty feed launches nothing
            got = t.feed_device(text.ptr + 1, len(fq), starts)
            assert t.finish()["n_bases"] == n_bases and t.timings()["feeds"] == 2
        _same_fields(got, want)
    finally:
        text.free()
    with lib().Trimmer(0) as t:                              # a stream of blank lines: no record, no base, no bits
        t.set_cover(np.zeros(0, dtype=np.uint8), 0)
        assert all(v.size == 0 for v in t.feed(b"\n\n\r\n", [4]).values())
        assert t.finish() == {"n_records": 0, "n_bases": 0, "n_covered": 0} and t.timings()["trim_s"] == 0


# ------------------------------------------------------------------ the threshold
@pytest.mark.parametrize("k", KS)
def test_threshold_and_the_base_count_guard(gpu, k):
    fq, bits, n_bases, want = _random_case(k, True, T)
    plain = _random_case(k, True, 0)
    assert 0 < n_bases < plain[2]                            # the threshold takes valid bases away
    tabs = gs.tables(k, 1, seed=710 + k)
    with Device(tabs) as dev, lib().QueryIndexer(k, device=0, fmt="fastq", min_qual_byte=T) as q:
        q.set_tables(dev.ptrs, 1, 255)
        assert stream(q, fq, cover=True, reset=False)["n_bases"] == n_bases      # phase 1 counts the same valid bases
    starts = trim_ref.starts(fq)
    with lib().Trimmer(0) as t:
        t.set_cover(bits, n_bases, T)
        _same_fields(_feed_all(t, fq, starts, 7), want)
        assert t.finish()["n_bases"] == n_bases
    biased = fastq_qual_ref.biased_qualities(_stream(k), T, 0.2, seed=9)
    base_rec = mask_ref.walk(trim_ref.fasta_of(biased, T), 1)[1]
    cover = trim_inputs.bits(np.bincount(base_rec, minlength=len(starts) - 1), seed=60 + k)
    with lib().Trimmer(0) as t:
        t.set_cover(mask_ref.pack(cover), int(cover.size), T)
        _same_fields(_feed_all(t, biased, trim_ref.starts(biased), None), trim_ref.runs(biased, cover, T=T))
        t.finish()
    with lib().Trimmer(0) as t:                              # bits made for the unmasked stream: another n_bases
        t.set_cover(plain[1], plain[2], T)
        _feed_all(t, fq, starts, None)
        with pytest.raises(lib().PkError) as exc:
            t.finish()
        assert exc.value.code == lib().PK_ERR_STATE and str(n_bases) in str(exc.value)


# ------------------------------------------------------------------ argument errors
def test_argument_errors_launch_nothing(gpu):
    L = lib()
    fq, bits, n_bases, want = _random_case(5, True, 0)
    starts = trim_ref.starts(fq)
    R = len(starts) - 1
    buf = np.frombuffer(fq, dtype=np.uint8)
    out = np.full((len(L.TRIM_FIELDS), R), gs.SENTINEL, dtype=np.uint64)
    with L.Trimmer(0) as t:
        t.set_cover(bits, n_bases)
        feed = L.load().pk_trim_feed
        swapped = starts.copy()
        swapped[[3, 4]] = swapped[[4, 3]]
        short = starts.copy()
        short[-1] -= np.uint64(1)
        for text_p, n, starts_p, out_p in ((buf.ctypes.data, len(fq), swapped.ctypes.data, out.ctypes.data),      # non-monotone
                                           (buf.ctypes.data, len(fq), short.ctypes.data, out.ctypes.data),        # last offset != length
                                           (buf.ctypes.data, len(fq) + 1, starts.ctypes.data, out.ctypes.data),
                                           (None, len(fq), starts.ctypes.data, out.ctypes.data),                  # null pointers with records
                                           (buf.ctypes.data, len(fq), None, out.ctypes.data),
                                           (buf.ctypes.data, len(fq), starts.ctypes.data, None)):
            assert feed(t._h, text_p, n, starts_p, R, out_p) == L.PK_ERR_ARG
        assert (out == gs.SENTINEL).all() and t.timings() == {"trim_s": 0.0, "feeds": 0}
        with pytest.raises(ValueError, match="must not decrease"):
            t.feed(buf, swapped)
        _same_fields(_feed_all(t, fq, starts, None), want)   # the stream did not move
        assert t.finish()["n_bases"] == n_bases
        assert feed(t._h, buf.ctypes.data, len(fq), starts.ctypes.data, R, out.ctypes.data) == L.PK_ERR_STATE         # finished
        assert L.load().pk_trim_set_cover(t._h, bits.ctypes.data, n_bases, 0) == L.PK_ERR_STATE
    assert ctypes.sizeof(ctypes.c_uint64) == 8


# ------------------------------------------------------------------ end to end
E2E = dict(n_reads=2000, length=150, sub_rate=0.005, genome_bp=30_000, k=11, min_count=2, min_len=100)


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """The read set, its mate, the table indexed from the first by indexer.py, and the references (computed once)."""
    tmp = tmp_path_factory.mktemp("trim_e2e")
    genome = np.random.default_rng(77).integers(0, 4, E2E["genome_bp"], dtype=np.uint8)
    fq1, fa1 = fastq_ref.read_set(E2E["n_reads"], E2E["length"], seed=11, sub_rate=E2E["sub_rate"], genome=genome)
    fq2, _ = fastq_ref.read_set(E2E["n_reads"], E2E["length"], seed=12, sub_rate=E2E["sub_rate"], genome=genome)
    (tmp / "reads_1.fq").write_bytes(fq1)
    (tmp / "reads_2.fq").write_bytes(fq2)
    run_py("indexer.py", str(tmp / "reads_1.fq"), "s", str(E2E["k"]), cwd=str(tmp))
    kin = f"{tmp / 'reads_1.fq'}.{E2E['k']:02d}.kin"
    table = oracle.count_fasta(fa1, E2E["k"])["table"]
    return tmp, kin, table, fq1, fq2


def _npz_equals(z, want, tag=""):
    for key in ("trim_start", "trim_end", "covered", "seq_len"):
        assert z[key + tag].dtype == np.uint64 and np.array_equal(z[key + tag], want[key]), key + tag


def test_trim_py_end_to_end(gpu, reads):
    tmp, kin, table, fq1, fq2 = reads
    k, L = E2E["k"], E2E["min_len"]
    want = trim_ref.runs(fq1, [table], k, E2E["min_count"], 255, fast=True)
    whole, cut, dropped = trim_ref.classes(want, L)
    assert min(whole, cut, dropped) >= 0.10, (whole, cut, dropped)
    keep = trim_ref.keep_of(want, L)
    r = run_py("trim.py", "clean", "reads_1.fq", kin, "--min-count", "2", "--min-len", str(L), cwd=str(tmp),
               env=dict(gs.env_without_ranks(), PK_FEED_PIECE=str(1 << 16)))                  # ten feeds, cut at record offsets
    trimmed = (tmp / "clean.trimmed.fq").read_bytes()
    assert trimmed == trim_ref.trimmed_bytes(fq1, want["trim_start"], want["trim_end"], keep)
    z = np.load(tmp / "clean.kmt")
    _npz_equals(z, want)
    assert np.array_equal(z["keep"], keep) and int(z["n_bases"]) == want["n_bases"] and int(z["min_len"]) == L
    meta = json.load(open(tmp / "clean.kmt.json"))
    length = (want["trim_end"] - want["trim_start"]).astype(np.int64)
    assert (meta["n_records"], meta["n_kept"], meta["bases_kept"]) == (E2E["n_reads"], int(keep.sum()), int(length[keep != 0].sum()))
    assert meta["trim_s"] > 0 and meta["lookup_s"] > 0 and meta["select_s"] > 0
    assert r.stdout.strip().split("\n")[-1].startswith(f"{int(keep.sum())} of {E2E['n_reads']} reads kept, {meta['n_trimmed']} of them trimmed, ")
    # the trimmed file is FASTQ still (line 4 as long as line 2), and indexer.py takes it
    fastq_ref.fastq_to_fasta(trimmed)
    run_py("indexer.py", "clean.trimmed.fq", "t", str(k), cwd=str(tmp))
    assert np.array_equal(np.fromfile(tmp / f"clean.trimmed.fq.{k:02d}.kin", dtype=np.uint8), oracle.count_fasta(fastq_ref.fastq_to_fasta(trimmed), k)["table"])


def test_trim_py_with_mate_rest_and_min_qual(gpu, reads):
    tmp, kin, table, fq1, fq2 = reads
    k = E2E["k"]
    w1, w2 = (trim_ref.runs(fq, [table], k, E2E["min_count"], 255, T=38, fast=True) for fq in (fq1, fq2))
    keep = trim_ref.keep_of(w1, 20) & trim_ref.keep_of(w2, 20)
    assert 0.1 < keep.mean() < 0.9 and w1["n_bases"] < trim_ref.runs(fq1, [table], k, E2E["min_count"], 255, fast=True)["n_bases"]
    run_py("trim.py", "pair", "reads_1.fq", kin, "--min-count", "2", "--min-len", "20", "--mate", "reads_2.fq", "--rest", "--min-qual", "5", cwd=str(tmp))
    for tag, fq, w in (("1", fq1, w1), ("2", fq2, w2)):
        assert (tmp / f"pair.trimmed_{tag}.fq").read_bytes() == trim_ref.trimmed_bytes(fq, w["trim_start"], w["trim_end"], keep), tag
        assert (tmp / f"pair.rest_{tag}.fq").read_bytes() == trim_ref.rest_bytes(fq, keep), tag
    z = np.load(tmp / "pair.kmt")
    _npz_equals(z, w1)
    _npz_equals(z, w2, "_2")
    assert np.array_equal(z["keep"], keep) and int(z["n_bases_2"]) == w2["n_bases"]
    meta = json.load(open(tmp / "pair.kmt.json"))
    assert (meta["min_qual"], meta["qual_offset"], meta["n_kept"]) == (5, 33, int(keep.sum()))
    r = run_py("trim.py", "no", "reads_1.fa", kin, cwd=str(tmp), status=1)                       # FASTA is refused, naming mask.py
    assert any(line.startswith("error: ") and "mask.py" in line for line in r.stderr.splitlines()) and not list(tmp.glob("no.*"))
