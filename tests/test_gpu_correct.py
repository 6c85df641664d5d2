"""GPU: the correct path -- the Corrector (kmer_correct.hip, pk_correct_*) against correct_ref with exact equality of the six
fields, the patched bytes and the totals: small dense tables at k = 5 and 7, whole and cut into feeds, host and device forms,
the threshold, bits from anywhere, the u32 and u64 instantiations at k = 15 and 17 on tables counted on the GPU -- planted
errors, and seam_inputs' enumeration of every candidate around the first step seam -- sixteen tables, the guards, and
correct.py end to end as a child process.  tests/test_correct_host.py holds correct_ref against hand-worked records and
asserts on the CPU that the inputs used here reach every outcome class and the seams of the kernel's 64-position steps."""
import contextlib
import functools
import gzip
import json
import types

import numpy as np
import pytest

import correct_inputs
import correct_ref
import fastq_qual_ref
import fastq_ref
import gpu_support as gs
import mask_ref
import oracle
import query_ref
import seam_inputs
import trim_inputs
import trim_ref
from gpu_support import Device, SentinelOut, lib, run_py, stream

pytestmark = pytest.mark.gpu
T = 53                                                       # the threshold byte of --min-qual 20 at offset 33
MS = (1, 2, None)


@functools.lru_cache(maxsize=None)
def _tables(k: int, n: int):
    return correct_inputs.tables(k, n, seed=800 + k)


@functools.lru_cache(maxsize=None)
def _stream(k: int, n: int, tq: int = 0) -> bytes:
    fq = correct_inputs.stream(k, _tables(k, n)[1], seed=810 + k, final_newline=(n == 1), blank_tail=(n == 1))
    return fastq_qual_ref.biased_qualities(fq, tq, 0.03, seed=5) if tq else fq


@functools.lru_cache(maxsize=None)
def _want(k: int, n: int, window, M, tq: int = 0):
    """The reference of a case: computed once, shared by the tests, never changed."""
    return correct_ref.expected(_stream(k, n, tq), k, _tables(k, n)[0], *window, M=M, T=tq)


def _feed_all(c, fq, starts, per):
    """The stream through a Corrector in feeds of `per` records (None: one feed): the feeds' fields and texts concatenated."""
    R = len(starts) - 1
    buf = np.frombuffer(fq, dtype=np.uint8)
    parts, texts = [], []
    for lo in range(0, max(R, 1), per or max(R, 1)):
        hi = min(R, lo + (per or R))
        a, b = int(starts[lo]), int(starts[hi])
        fields, text = c.feed(buf[a:b], starts[lo:hi + 1] - starts[lo])
        parts.append(fields)
        texts.append(text.tobytes())
    return {name: np.concatenate([p[name] for p in parts]) for name in lib().CORR_FIELDS}, b"".join(texts)


def _same(got, text, want):
    for name in correct_ref.FIELDS:
        assert got[name].dtype == np.uint64 and got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape)
        assert np.array_equal(got[name], want[name]), (name, np.flatnonzero(got[name] != want[name])[:8], got[name][:8], want[name][:8])
    if text != want["patched"]:
        a, b = np.frombuffer(text, dtype=np.uint8), np.frombuffer(want["patched"], dtype=np.uint8)
        assert a.shape == b.shape, (a.shape, b.shape)
        at = np.flatnonzero(a != b)
        raise AssertionError(("patched bytes", at[:8], a[at[:8]], b[at[:8]]))


# ------------------------------------------------------------------ small dense tables, every setting
@pytest.mark.parametrize("k", [5, 7])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("window", [(1, 255), (2, 254)])
def test_corrector_against_the_reference(gpu, k, n, window):
    fq = _stream(k, n)
    starts = trim_ref.starts(fq)
    with Device(_tables(k, n)[0]) as dev:
        for M in MS:
            want = _want(k, n, window, M)
            assert int(want["corrected"].sum()) > 0 and int(want["unfixable"].sum()) > 0 and int(want["untried"].sum()) > (0 if M != 1 else -1)
            for per in (None, 1, 2, 7):
                with lib().Corrector(k, 0) as c:
                    c.set_tables(dev.ptrs, *window)
                    c.set_cover(want["bits"], want["n_bases"], 0, M)
                    got, text = _feed_all(c, fq, starts, per)
                    fin = c.finish()
                    timings = c.timings()
                _same(got, text, want)
                assert fin == correct_ref.totals(want), (M, per)
                assert timings["correct_s"] > 0 and timings["feeds"] == (1 if per is None else -(-(len(starts) - 1) // per))


def test_device_form_threshold_and_empty_feeds(gpu):
    k, n = 7, 3
    fq = _stream(k, n, T)
    want = _want(k, n, (1, 255), 2, T)
    plain = _want(k, n, (1, 255), 2)
    assert 0 < want["n_bases"] < plain["n_bases"] and int(want["corrected"].sum()) > 0          # the threshold takes valid bases away
    starts = trim_ref.starts(fq)
    text = lib().DeviceBuffer(len(fq) + 1, 0)
    out = lib().DeviceBuffer(len(fq) + 3, 0)
    try:
        text.upload(np.frombuffer(b"x" + fq, dtype=np.uint8))            # the text and its copy at odd addresses
        with Device(_tables(k, n)[0]) as dev:
            with lib().QueryIndexer(k, device=0, fmt="fastq", min_qual_byte=T) as q:              # the bits of the lookup itself
                q.set_tables(dev.ptrs, 1, 255)
                cover = stream(q, fq, cover=True, reset=False)
            assert cover["n_bases"] == want["n_bases"] and np.array_equal(cover["bits"], want["bits"])
            with lib().Corrector(k, 0) as c:
                c.set_tables(dev.ptrs, 1, 255)
                c.set_cover(cover["bits"], cover["n_bases"], T, 2)
                fields, empty = c.feed(b"", [0])                         # an empty feed launches nothing
                assert all(v.size == 0 for v in fields.values()) and empty.size == 0
                got = c.feed_device(text.ptr + 1, len(fq), starts, out.ptr + 3)
                assert c.finish() == correct_ref.totals(want) and c.timings()["feeds"] == 2
            _same(got, out.download()[3:].tobytes(), want)
            assert text.download()[1:].tobytes() == fq               # the text that is read is never written
            with lib().Corrector(k, 0) as c:                             # the host form under the threshold, in feeds of 7
                c.set_tables(dev.ptrs, 1, 255)
                c.set_cover(want["bits"], want["n_bases"], T, 2)
                _same(*_feed_all(c, fq, starts, 7), want)
                c.finish()
            with lib().Corrector(k, 0) as c:                             # a stream of blank lines: no record, no base, no bits
                c.set_tables(dev.ptrs, 1, 255)
                c.set_cover(np.zeros(0, dtype=np.uint8), 0)
                fields, same = c.feed(b"\n\n\r\n", [4])
                assert all(v.size == 0 for v in fields.values()) and same.tobytes() == b"\n\n\r\n"
                assert c.finish() == {"n_records": 0, "n_bases": 0, "n_candidates": 0, "n_untried": 0, "n_corrected": 0, "n_ambiguous": 0}
                assert c.timings()["correct_s"] == 0
    finally:
        text.free()
        out.free()


@pytest.mark.parametrize("k", [5, 7])
def test_bits_from_anywhere(gpu, k):
    """Cover bits that no table made: candidates in the middle of long runs, covered bases whose windows do not match."""
    n = 3
    fq = _stream(k, n)
    starts = trim_ref.starts(fq)
    cover = trim_inputs.bits(_want(k, n, (1, 255), 1)["n_valid_bases"], seed=60 + k)
    with Device(_tables(k, n)[0]) as dev:
        for M in MS:
            want = correct_ref.expected(fq, k, _tables(k, n)[0], M=M, cover=cover)
            assert int(want["corrected"].sum()) > 0 and int(want["ambiguous"].sum()) > 0
            with lib().Corrector(k, 0) as c:
                c.set_tables(dev.ptrs, 1, 255)
                c.set_cover(mask_ref.pack(cover), int(cover.size), 0, M)
                _same(*_feed_all(c, fq, starts, 7), want)
                assert c.finish() == correct_ref.totals(want)


# ------------------------------------------------------------------ k = 15 and 17: the u32 and u64 instantiations
@contextlib.contextmanager
def _counted(k):
    """The counted tables of k (three, at k = 17 two of 16 GiB) in their indexers, as test_gpu_query_reads.py builds them."""
    sources, sparse = query_ref.counted_case(k)
    with contextlib.ExitStack() as stack:
        ptrs = []
        for src in sources:
            ix = stack.enter_context(lib().Indexer(k, device=0))
            ix.feed(src)
            ix.finish()
            ptrs.append(ix.table_device_ptr())
        yield types.SimpleNamespace(k=k, ptrs=ptrs, sparse=sparse, sources=sources)


@pytest.fixture(scope="module")
def k15(gpu):
    with _counted(15) as c:
        yield c


@pytest.fixture(scope="module")
def k17(gpu):
    with _counted(17) as c:
        yield c


@pytest.mark.parametrize("k", [15, 17])
def test_counted_tables_and_planted_errors(request, k):
    at_k = request.getfixturevalue(f"k{k}")
    clean = query_ref.reads_from(at_k.sources, k, 1500, seed=1700 + k, fastq=True)
    fq, offs, _ = correct_inputs.plant(clean, 0.01, seed=1800 + k)
    starts = trim_ref.starts(fq)
    for window, M in (((1, 255), None), ((2, 254), k)):      # the default; and only candidates with all k windows: 3 k lanes
        want = correct_ref.expected(fq, k, at_k.sparse, *window, M=M)
        assert int(want["corrected"].sum()) > 0 and offs.size > 100
        with lib().Corrector(k, 0) as c:
            c.set_tables(at_k.ptrs, *window)
            c.set_cover(want["bits"], want["n_bases"], 0, M)
            _same(*_feed_all(c, fq, starts, 400), want)
            assert c.finish() == correct_ref.totals(want)


@pytest.mark.parametrize("k", [15, 17])
def test_counted_tables_at_the_first_step_seam(request, k):
    """seam_inputs.correct_cases on the u32 kernel's widest k and on the u64 kernel: every candidate position around position
    64 with every distance to an N below and above it, reads cut from the first counted source."""
    at_k = request.getfixturevalue(f"k{k}")
    fq, cover, cases = seam_inputs.correct_cases(k, 64, query_ref.sequence(at_k.sources[0]), "N", seed=1900 + k)
    starts = trim_ref.starts(fq)
    assert len(starts) - 1 == len(cases) == (2 * k + 2) * (k + 1) ** 2
    want = correct_ref.expected(fq, k, at_k.sparse, M=1, cover=cover)       # M = 1: every window count 1 .. k is tried, 3 k lanes at the most
    assert np.array_equal(want["candidates"], np.array([seam_inputs.is_candidate(k, a, b) for _, a, b in cases], dtype=np.uint64))
    assert int(want["untried"].sum()) == 0 and int(want["corrected"].sum()) >= 0.9 * int(want["candidates"].sum())
    with lib().Corrector(k, 0) as c:
        c.set_tables(at_k.ptrs, 1, 255)
        c.set_cover(mask_ref.pack(cover), int(cover.size), 0, 1)
        _same(*_feed_all(c, fq, starts, 1000), want)
        assert c.finish() == correct_ref.totals(want)


# ------------------------------------------------------------------ sixteen tables: the limit of one correction
def test_sixteen_tables_each_with_a_sixteenth_of_the_kmers(gpu):
    """A candidate's windows match in different tables, some in the sixteenth only: the gather loop runs to its last table."""
    k = 5
    tabs, _ = seam_inputs.sixteen_tables(k)
    fq = seam_inputs.sixteen_stream(k)
    starts = trim_ref.starts(fq)
    assert len(tabs) == 16
    with Device(tabs) as dev:
        for M in (1, None):
            want = correct_ref.expected(fq, k, tabs, M=M)
            less = correct_ref.expected(fq, k, tabs[:-1], M=M)
            assert int(want["corrected"].sum()) >= 10 and want["patched"] != less["patched"]     # the last table changes the result
            for per in (None, 7):
                with lib().Corrector(k, 0) as c:
                    c.set_tables(dev.ptrs, 1, 255)
                    c.set_cover(want["bits"], want["n_bases"], 0, M)
                    _same(*_feed_all(c, fq, starts, per), want)
                    assert c.finish() == correct_ref.totals(want)
            with lib().QueryIndexer(k, device=0, fmt="fastq") as q:       # the lookup's bits over the same sixteen
                q.set_tables(dev.ptrs, 1, 255)
                cover = stream(q, fq, cover=True, reset=False)
            assert cover["n_bases"] == want["n_bases"] and np.array_equal(cover["bits"], want["bits"])


# ------------------------------------------------------------------ guards
def test_guards_launch_nothing(gpu):
    L = lib()
    k, n = 5, 1
    fq = _stream(k, n)
    want = _want(k, n, (1, 255), 2)
    starts = trim_ref.starts(fq)
    R = len(starts) - 1
    buf = np.frombuffer(fq, dtype=np.uint8)
    out = np.full((len(L.CORR_FIELDS), R), gs.SENTINEL, dtype=np.uint64)
    text = L.DeviceBuffer(len(fq), 0)
    text.upload(buf)
    sent = SentinelOut(text_out=len(fq))
    try:
        with Device(_tables(k, n)[0]) as dev, L.Corrector(k, 0) as c:
            feed = L.load().pk_correct_feed_device
            args = (text.ptr, len(fq), starts.ctypes.data, R, sent.text_out.ptr, out.ctypes.data)
            assert feed(c._h, *args) == L.PK_ERR_STATE                                  # no tables, no bits
            assert L.load().pk_correct_set_cover(c._h, want["bits"].ctypes.data, want["n_bases"], 0, 2) == L.PK_ERR_STATE
            c.set_tables(dev.ptrs, 1, 255)
            assert feed(c._h, *args) == L.PK_ERR_STATE                                  # tables, no bits
            for tq, M in ((256, 2), (-1, 2), (0, 0), (0, k + 1)):
                assert L.load().pk_correct_set_cover(c._h, want["bits"].ctypes.data, want["n_bases"], tq, M) == L.PK_ERR_ARG
            assert L.load().pk_correct_set_cover(c._h, None, want["n_bases"], 0, 2) == L.PK_ERR_ARG
            assert feed(c._h, *args) == L.PK_ERR_STATE
            c.set_cover(want["bits"], want["n_bases"], 0, 2)
            swapped = starts.copy()
            swapped[[3, 4]] = swapped[[4, 3]]
            short = starts.copy()
            short[-1] -= np.uint64(1)
            for text_p, nb, starts_p, out_text_p, out_p in ((text.ptr, len(fq), swapped.ctypes.data, sent.text_out.ptr, out.ctypes.data),   # non-monotone
                                                            (text.ptr, len(fq), short.ctypes.data, sent.text_out.ptr, out.ctypes.data),     # last offset != length
                                                            (text.ptr, len(fq) + 1, starts.ctypes.data, sent.text_out.ptr, out.ctypes.data),
                                                            (None, len(fq), starts.ctypes.data, sent.text_out.ptr, out.ctypes.data),        # null pointers
                                                            (text.ptr, len(fq), None, sent.text_out.ptr, out.ctypes.data),
                                                            (text.ptr, len(fq), starts.ctypes.data, None, out.ctypes.data),
                                                            (text.ptr, len(fq), starts.ctypes.data, sent.text_out.ptr, None),
                                                            (text.ptr, len(fq), starts.ctypes.data, text.ptr + 1, out.ctypes.data)):       # overlapping texts
                assert feed(c._h, text_p, nb, starts_p, R, out_text_p, out_p) == L.PK_ERR_ARG
            assert (out == gs.SENTINEL).all() and sent.untouched() and c.timings() == {"correct_s": 0.0, "feeds": 0}
            _same(*_feed_all(c, fq, starts, None), want)         # the stream did not move
            assert c.finish() == correct_ref.totals(want)
            assert feed(c._h, *args) == L.PK_ERR_STATE                                  # finished
            assert L.load().pk_correct_set_tables(c._h, (L.ctypes.c_void_p * 1)(dev.ptrs[0]), 1, 1, 255) == L.PK_ERR_STATE
            assert sent.untouched()
        other = _want(7, 1, (1, 255), 2)                         # bits made for another stream: another n_bases
        assert other["n_bases"] != want["n_bases"]
        with Device(_tables(k, n)[0]) as dev, L.Corrector(k, 0) as c:
            c.set_tables(dev.ptrs, 1, 255)
            c.set_cover(other["bits"], other["n_bases"], 0, 2)
            _feed_all(c, fq, starts, None)
            with pytest.raises(L.PkError) as exc:
                c.finish()
            assert exc.value.code == L.PK_ERR_STATE and str(want["n_bases"]) in str(exc.value)
    finally:
        text.free()
        sent.free()


# ------------------------------------------------------------------ end to end
E2E = dict(n_reads=600, length=150, sub_rate=0.01, genome_bp=10_000, k=11, min_count=2)


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """The read set, plain and gzipped, the table indexed from it by indexer.py, and the oracle's table."""
    tmp = tmp_path_factory.mktemp("correct_e2e")
    genome = np.random.default_rng(78).integers(0, 4, E2E["genome_bp"], dtype=np.uint8)
    fq, fa = fastq_ref.read_set(E2E["n_reads"], E2E["length"], seed=13, sub_rate=E2E["sub_rate"], genome=genome)
    fq = fastq_qual_ref.biased_qualities(fq, T, 0.02, seed=14)
    (tmp / "reads.fq").write_bytes(fq)
    with gzip.open(tmp / "packed.fq.gz", "wb") as fh:
        fh.write(fq)
    run_py("indexer.py", str(tmp / "reads.fq"), "s", str(E2E["k"]), cwd=str(tmp))
    kin = f"{tmp / 'reads.fq'}.{E2E['k']:02d}.kin"
    return tmp, kin, oracle.count_fasta(fa, E2E["k"])["table"], fq


def _check_run(tmp, name, r, fq, want, M, reads_file):
    assert (tmp / f"{name}.corrected.fq").read_bytes() == want["patched"]
    z = np.load(tmp / f"{name}.kme")
    for key in ("candidates", "untried", "corrected", "ambiguous", "seq_len", "fix_record", "fix_pos"):
        assert z[key].dtype == np.uint64 and np.array_equal(z[key], want[key]), key
    for key in ("fix_old", "fix_new"):
        assert z[key].dtype == np.uint8 and np.array_equal(z[key], want[key]), key
    assert (int(z["kmer_len"]), int(z["min_count"]), int(z["min_windows"]), int(z["n_bases"])) == (E2E["k"], E2E["min_count"], M, want["n_bases"])
    meta = json.load(open(tmp / f"{name}.kme.json"))
    t = correct_ref.totals(want)
    assert (meta["n_records"], meta["n_candidates"], meta["n_untried"], meta["n_corrected"], meta["n_ambiguous"], meta["n_unfixable"]) == \
        (E2E["n_reads"], t["n_candidates"], t["n_untried"], t["n_corrected"], t["n_ambiguous"], int(want["unfixable"].sum()))
    assert meta["bytes"] == len(fq) and meta["output"] == f"{name}.corrected.fq" and meta["query_file"] == reads_file
    assert meta["correct_s"] > 0 and meta["lookup_s"] > 0 and meta["min_windows"] == M
    assert r.stdout.strip().split("\n")[-1] == (
        f"{t['n_corrected']} bases corrected in {int((want['corrected'] > 0).sum())} of {E2E['n_reads']} reads "
        f"({t['n_candidates']} candidates: {t['n_untried']} untried, {t['n_ambiguous']} ambiguous, {int(want['unfixable'].sum())} unfixable), {name}.corrected.fq")
    return meta


def test_correct_py_end_to_end(gpu, reads):
    tmp, kin, table, fq = reads
    k = E2E["k"]
    want = correct_ref.expected(fq, k, [table], E2E["min_count"], 255)
    assert int(want["corrected"].sum()) > 100 and int(want["untried"].sum()) > 0
    r = run_py("correct.py", "fixed", "reads.fq", kin, "--min-count", "2", cwd=str(tmp),
               env=dict(gs.env_without_ranks(), PK_FEED_PIECE=str(1 << 16)))                      # several feeds, cut at record offsets
    meta = _check_run(tmp, "fixed", r, fq, want, (k + 1) // 2, "reads.fq")
    assert "min_qual" not in meta
    fastq_ref.fastq_to_fasta((tmp / "fixed.corrected.fq").read_bytes())          # FASTQ still
    r = run_py("correct.py", "packed", "packed.fq.gz", kin, "--min-count", "2", cwd=str(tmp))    # a .fq.gz input: the same output bytes
    _check_run(tmp, "packed", r, fq, want, (k + 1) // 2, "packed.fq.gz")
    r = run_py("correct.py", "no", "reads.fa", kin, cwd=str(tmp), status=1)                       # FASTA is refused
    assert any(line.startswith("error: ") for line in r.stderr.splitlines()) and not list(tmp.glob("no.*"))


def test_correct_py_with_min_qual(gpu, reads):
    tmp, kin, table, fq = reads
    want = correct_ref.expected(fq, E2E["k"], [table], E2E["min_count"], 255, M=3, T=T)
    plain = correct_ref.expected(fq, E2E["k"], [table], E2E["min_count"], 255, M=3)
    assert int(want["corrected"].sum()) > 0 and want["n_bases"] < plain["n_bases"] and want["patched"] != plain["patched"]
    r = run_py("correct.py", "qual", "reads.fq", kin, "--min-count", "2", "--min-windows", "3", "--min-qual", "20", cwd=str(tmp))
    meta = _check_run(tmp, "qual", r, fq, want, 3, "reads.fq")
    assert (meta["min_qual"], meta["qual_offset"]) == (20, 33)
