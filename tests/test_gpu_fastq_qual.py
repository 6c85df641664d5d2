"""GPU: base qualities (pk_indexer_set_min_qual, k_fq_mask in fastq.hip).  A FASTQ stream under the threshold byte T is counted
exactly like the FASTA text fastq_qual_ref.mask_fastq_to_fasta makes of it -- by the oracle, or at k = 15 by the GPU FASTA
path -- however the stream is cut into feeds; every comparison is exact."""
import functools
import gzip
import json
import types

import numpy as np
import pytest

import gpu_support as gs
import fastq_ref
import oracle
import query_ref
from fastq_qual_ref import biased_qualities, hand_qualities, mask_fastq_to_fasta
from fastq_ref import CASES
from gpu_support import Device, feed, lib, record_names, run_py

pytestmark = pytest.mark.gpu
THRESHOLDS = [1, 34, 53, 255]


def _finish(ix, fastq: bool = True):
    fin = ix.finish()
    fin["records"] = ix.records(fin["n_records"])
    fin["table"] = ix.table_to_host()
    if fastq:
        fin["stats"], fin["masked"] = ix.fastq_stats(), ix.fastq_masked()
    return fin


def _count(fq: bytes, k: int, T: int, cuts=None, ix=None):
    """FASTQ under threshold byte T, fed whole or in pieces; through `ix` (which is reset behind it) or an indexer of its own."""
    if ix is not None:
        feed(ix, fq, cuts)
        fin = _finish(ix)
        ix.reset()
        return fin
    with lib().Indexer(k, device=0, fmt="fastq", min_qual_byte=T) as own:
        feed(own, fq, cuts)
        return _finish(own)


def _check(got, fq: bytes, k: int, T: int, want=None):
    """`got` against the oracle (or `want`, a count of the same text) on the masked FASTA text."""
    fa, n_masked = mask_fastq_to_fasta(fq, T)
    want = want or oracle.count_fasta(fa, k)
    assert got["masked"] == n_masked
    assert got["num_kmers"] == want["num_kmers"] and got["total_bp"] == want["total_bp"]
    assert np.array_equal(got["table"], want["table"])
    hist = want["hist256"][1:] if "hist256" in want else oracle.table_stats(want["table"])[0]
    assert np.array_equal(got["hist256"][1:], hist)
    assert got["n_records"] == len(want["records"])
    assert record_names(fq, got["records"]) == record_names(fa, want["records"])
    assert got["stats"] == fastq_ref.stats(fq)


def _same(a, b):
    for key in ("num_kmers", "total_bp", "n_records", "stats", "masked"):
        assert a[key] == b[key], key
    assert np.array_equal(a["table"], b["table"]) and np.array_equal(a["hist256"], b["hist256"])
    assert np.array_equal(a["records"], b["records"])


# ------------------------------------------------------------------ hand cases ---------------------
LOW_BLANKS = b"@blanks under low qualities\n \tAC GT\x1f \n+\n!!!!!!!!!\n"
ALONE = [(name, fq) for name, fq, _ in CASES if fq] + [("low_blanks", LOW_BLANKS)]


def _stream(eol: bytes) -> bytes:
    """The hand-written cases whose lines end in "\\n", in one stream with the terminator `eol`: an empty read, blanks under
    what will be low qualities, and last a read without a final newline."""
    names = ("plain", "empty_reads", "quality_starts_with_at_plus_gt", "quality_all_acgt", "name_with_blanks_and_tabs", "lower_case_and_n",
             "seq_with_leading_blank", "no_final_newline")
    by_name = {name: fq for name, fq, _ in CASES}
    parts = [by_name[n] for n in names[:-1]] + [LOW_BLANKS, by_name[names[-1]]]
    return b"".join(parts).replace(b"\n", eol)


@pytest.mark.parametrize("T", THRESHOLDS)
def test_each_hand_case_alone(gpu, T):
    with lib().Indexer(7, device=0, fmt="fastq", min_qual_byte=T) as ix:
        for i, (name, fq) in enumerate(ALONE):
            fq = hand_qualities(fq, T, seed=100 * T + i)
            _check(_count(fq, 7, T, ix=ix), fq, 7, T)


@pytest.mark.parametrize("eol", [b"\n", b"\r\n", b"\r"], ids=["lf", "crlf", "cr"])
@pytest.mark.parametrize("T", THRESHOLDS)
def test_hand_cases_in_one_stream(gpu, T, eol):
    fq = hand_qualities(_stream(eol), T, seed=T)
    assert fastq_ref.stats(fq)["records"] == 16
    got = _count(fq, 7, T)
    _check(got, fq, 7, T)
    assert got["masked"] > 10


# ------------------------------------------------------------------ cuts ---------------------------
@pytest.mark.parametrize("T", [53, 255])
def test_cuts_give_identical_results(gpu, T):
    fq = hand_qualities(_stream(b"\r\n"), T, seed=7)
    assert 300 < len(fq) < 1000
    rng = np.random.default_rng(T)
    with lib().Indexer(7, device=0, fmt="fastq", min_qual_byte=T) as ix:
        whole = _count(fq, 7, T, ix=ix)
        _check(whole, fq, 7, T)
        _same(_count(fq, 7, T, cuts=range(1, len(fq)), ix=ix), whole)          # one byte per feed
        for _ in range(20):
            cuts = sorted(int(c) for c in rng.integers(1, len(fq), int(rng.integers(1, 30))))
            _same(_count(fq, 7, T, cuts=cuts, ix=ix), whole)


# ------------------------------------------------------------------ lines 2 and 4 far apart --------
def test_long_read_quality_many_feeds_behind_its_bases(gpu):
    """A 40 000-base read on one line (three 16 KiB chunks per line) and a short one: line 4 arrives ten feeds of 4 096 bytes
    behind the bases it masks, or is cut a byte either side of every line's start and end."""
    k, T = 15, 53
    rng = np.random.default_rng(40)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 40_000)]
    fq = b"@long read\n" + seq.tobytes() + b"\n+\n" + b"I" * seq.size + b"\n@short\nACGTACGTAAACCCGTTGCA\n+\nIIIIIIIIII!!!!!IIIII\n"
    fq = biased_qualities(fq, T, 0.3, seed=41)
    fa, n_masked = mask_fastq_to_fasta(fq, T)
    assert 10_000 < n_masked < 14_000
    with lib().Indexer(k, device=0) as ref:                               # the GPU FASTA path on the masked text
        ref.feed(fa)
        want = _finish(ref, fastq=False)
    edges = sorted({c for s, e, t in fastq_ref.lines(fq) for x in (s, e, t) for c in (x - 1, x, x + 1) if 0 < c < len(fq)})
    with lib().Indexer(k, device=0, fmt="fastq", min_qual_byte=T) as ix:
        for cuts in (None, range(4096, len(fq), 4096), edges):
            _check(_count(fq, k, T, cuts=cuts, ix=ix), fq, k, T, want=want)


# ------------------------------------------------------------------ chunk seams, invariants --------
@functools.lru_cache(maxsize=None)
def _seam_set(T: int) -> bytes:
    """97 KB, six 16 KiB chunks; about 30 % of the qualities below T (T = 0: the set for T = 53, nothing is masked)."""
    fq, _ = fastq_ref.read_set(300, length=150, seed=12, genome_bp=20_000)
    return biased_qualities(fq, T or 53, 0.3, seed=13)


@functools.lru_cache(maxsize=None)
def _seam_count(T: int, quals_of: int, two_feeds: bool = False):
    fq = _seam_set(quals_of)
    return _count(fq, 9, T, cuts=[len(fq) // 2 + 5] if two_feeds else None)


@pytest.mark.parametrize("T", [34, 53])
def test_chunk_seams(gpu, T):
    fq = _seam_set(T)
    assert -(-len(fq) // 16384) == 6
    whole = _seam_count(T, T)
    _check(whole, fq, 9, T)
    assert 0.25 * 45_000 < whole["masked"] < 0.35 * 45_000
    _same(_seam_count(T, T, two_feeds=True), whole)


@pytest.mark.parametrize("T", [34, 53])
def test_only_the_valid_windows_change(gpu, T):
    masked, plain = _seam_count(T, T), _seam_count(0, T)
    fq = _seam_set(T)
    assert plain["masked"] == 0 and plain["stats"] == masked["stats"]
    for f in ("name_off", "name_len", "seq_len"):
        assert np.array_equal(masked["records"][f], plain["records"][f]), f
    assert [n for n, _, _ in record_names(fq, masked["records"])] == [n for n, _, _ in record_names(fq, plain["records"])]
    assert np.all(masked["records"]["n_valid_kmers"] <= plain["records"]["n_valid_kmers"])
    assert masked["num_kmers"] < plain["num_kmers"] and masked["total_bp"] == plain["total_bp"]


# ------------------------------------------------------------------ record-array growth ------------
def test_the_count_stays_exact_when_the_front_end_runs_twice(gpu):
    """3 000 reads of 1 to 3 bases in one feed need more record slots than bytes / 256 + 1024: the record array grows and the
    front end, the mask kernel with it, runs a second time over the feed."""
    rng = np.random.default_rng(3)
    T = 53
    recs = []
    for i in range(3000):
        n = int(rng.integers(1, 4))
        recs.append(b"@%d\n" % i + bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n)) + b"\n+\n" + b"I" * n + b"\n")
    fq = biased_qualities(b"".join(recs), T, 0.4, seed=4)
    assert 3000 > len(fq) // 256 + 1024
    got = _count(fq, 3, T)
    _check(got, fq, 3, T)
    assert 1500 < got["masked"] < 3500


# ------------------------------------------------------------------ malformed input ----------------
@pytest.mark.parametrize("surplus", [1, 100])
def test_a_quality_line_longer_than_its_bases(gpu, surplus):
    """Line 4 of record 2 is longer than line 2, all of it low: the same error as without masking, and the surplus bytes
    reach no text -- after a reset a good file counts right on the same buffers."""
    lib = gs.lib()
    T = 53
    fq = b"@r1\nACGTACGTACGT\n+\n!!!!!!!!!!!!\n@r2\nACGTAC\n+\n" + b"!" * (6 + surplus) + b"\n@r3\nACGTACGTAA\n+\n!!!!!!!!!!\n"
    want = fastq_ref.FastqError(2, fq.index(b"@r2"), 4)
    good = biased_qualities(fastq_ref.read_set(40, length=50, seed=2, genome_bp=2000)[0], T, 0.3, seed=5)
    messages = []
    for masked in (False, True):
        for bytewise in (False, True):
            with lib.Indexer(7, device=0, fmt="fastq", min_qual_byte=T if masked else 0) as ix:
                with pytest.raises(lib.PkError) as e:
                    feed(ix, fq, range(1, len(fq)) if bytewise else None)
                    ix.finish()
                assert e.value.code == lib.PK_ERR_FORMAT and str(want) in str(e.value), str(e.value)
                messages.append(str(e.value))
                ix.reset()
                _check(_count(good, 7, T if masked else 0, ix=ix), good, 7, T if masked else 0)
    assert len(set(messages)) == 1


# ------------------------------------------------------------------ off is off, state rules --------
def test_off_is_off(gpu):
    lib = gs.lib()
    fq = _seam_set(0)
    with lib.Indexer(9, device=0, fmt="fastq") as never:
        feed(never, fq)
        want = _finish(never)
    got = _count(fq, 9, 0)
    with lib.Indexer(9, device=0, fmt="fastq", min_qual_byte=53) as ix:     # set, then set back before the first feed
        lib._check(lib.load().pk_indexer_set_min_qual(ix._h, 0))
        _same(_count(fq, 9, 0, ix=ix), want)
    _same(got, want)
    assert got["masked"] == 0
    _check(got, fq, 9, 0)


def test_state_rules(gpu):
    lib = gs.lib()
    set_min_qual = lib.load().pk_indexer_set_min_qual
    fq = biased_qualities(fastq_ref.read_set(10, length=30, seed=1, genome_bp=1000)[0], 53, 0.3, seed=6)
    with lib.Indexer(7, device=0) as ix:                                     # a FASTA indexer
        assert set_min_qual(ix._h, 53) == lib.PK_ERR_STATE
        with pytest.raises(lib.PkError):
            ix.fastq_masked()
    with pytest.raises(ValueError):
        lib.Indexer(7, device=0, fmt="fastq", min_qual_byte=256)
    with lib.Indexer(7, device=0, fmt="fastq") as ix:
        assert set_min_qual(ix._h, 256) == lib.PK_ERR_ARG and set_min_qual(ix._h, -1) == lib.PK_ERR_ARG
        assert ix.fastq_masked() == 0
        lib._check(set_min_qual(ix._h, 255))
        lib._check(set_min_qual(ix._h, 53))
        ix.feed(fq[:100])
        assert set_min_qual(ix._h, 34) == lib.PK_ERR_STATE                 # after the first feed
        ix.feed(fq[100:])
        first = _finish(ix)
        _check(first, fq, 7, 53)
        assert set_min_qual(ix._h, 34) == lib.PK_ERR_STATE                 # and after finish
        ix.reset()                                                         # the threshold stays
        assert ix.fastq_masked() == 0
        _same(_count(fq, 7, 53, ix=ix), first)
        lib._check(set_min_qual(ix._h, 34))                                # a reset indexer takes a new one
        _check(_count(fq, 7, 34, ix=ix), fq, 7, 34)


# ------------------------------------------------------------------ query --------------------------
def test_query_masks_like_the_indexer(gpu, tmp_path):
    from pykmer_amd import query
    k, W, Q = 7, 5, 20
    fq = hand_qualities(_stream(b"\n"), Q + 33, seed=8) + b"\n" + biased_qualities(fastq_ref.read_set(60, length=80, seed=9, genome_bp=3000)[0], Q + 33, 0.3, seed=10)
    fa, n_masked = mask_fastq_to_fasta(fq, Q + 33)
    (tmp_path / "q.fq").write_bytes(fq)
    (tmp_path / "masked.fa").write_bytes(fa)
    dense = query_ref.random_tables(k, 3, 77)
    tables = [types.SimpleNamespace(kmer_len=k, index_file=f"t{i}.kin", data_size=4 ** k, table=t) for i, t in enumerate(dense)]

    def stage(group, device):
        dev = Device([g.table for g in group])
        return query.Staged(dev.ptrs, dev.bufs)

    got = query.query_records(str(tmp_path / "q.fq"), tables, 1, 255, device=0, stage=stage, min_qual=Q, bin_windows=W, coords=True)
    want = query.query_records(str(tmp_path / "masked.fa"), tables, 1, 255, device=0, stage=stage, bin_windows=W, coords=True)
    plain = query.query_records(str(tmp_path / "q.fq"), tables, 1, 255, device=0, stage=stage, bin_windows=W, coords=True)
    assert got["masked"] == n_masked > 500 and (got["min_qual"], got["qual_offset"]) == (Q, 33)
    assert "masked" not in plain and "min_qual" not in plain and "min_qual" not in want
    arrays = [key for key, v in want.items() if isinstance(v, np.ndarray)]
    assert set(arrays) >= {"hits", "depth", "n_valid", "seq_len", "bin_hits", "bin_depth", "bin_first", "bin_start", "bin_end"}
    for key in arrays:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert got["names"] == want["names"] == plain["names"] and got["num_kmers"] == want["num_kmers"] < plain["num_kmers"]
    assert np.array_equal(got["seq_len"], plain["seq_len"])


# ------------------------------------------------------------------ CLI ----------------------------
def test_indexer_cli(gpu, tmp_path):
    Q = 20
    fq = biased_qualities(fastq_ref.read_set(200, length=100, seed=6, genome_bp=5000)[0], Q + 33, 0.3, seed=11)
    fa, n_masked = mask_fastq_to_fasta(fq, Q + 33)
    (tmp_path / "masked.fa").write_bytes(fa)
    (tmp_path / "reads.fq").write_bytes(fq)
    with gzip.open(tmp_path / "reads.fq.gz", "wb") as fh:
        fh.write(fq)
    out = run_py("indexer.py", "masked.fa", "s", "7", cwd=str(tmp_path)).stdout
    assert "MASKED" not in out
    want = json.loads((tmp_path / "masked.fa.07.kin.json").read_text())
    kin = (tmp_path / "masked.fa.07.kin").read_bytes()
    for name, argv in (("reads.fq", ["reads.fq", "s", "7", "--min-qual", str(Q)]), ("reads.fq.gz", ["--min-qual", str(Q), "reads.fq.gz", "--qual-offset=33", "7"])):
        out = run_py("indexer.py", *argv, cwd=str(tmp_path)).stdout
        assert f"MASKED {n_masked} bases below quality {Q} (offset 33)\n" in out
        got = json.loads((tmp_path / f"{name}.07.kin.json").read_text())
        assert sorted(got) == sorted(want)                                 # the reference's keys, no new one
        for key in fastq_ref.DETERMINISTIC:
            assert got[key] == want[key], (name, key)
        assert (tmp_path / f"{name}.07.kin").read_bytes() == kin
    before = sorted(p.name for p in tmp_path.iterdir())
    r = run_py("indexer.py", "masked.fa", "t", "9", "--min-qual", str(Q), cwd=str(tmp_path), status=1)
    assert any(line.startswith("error: ") for line in r.stderr.splitlines()) and sorted(p.name for p in tmp_path.iterdir()) == before
