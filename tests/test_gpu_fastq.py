"""GPU: FASTQ input (fastq.hip) counted exactly like the FASTA text it stands for (fastq_ref.fastq_to_fasta)."""
import gzip
import json

import numpy as np
import pytest

import gpu_support as gs
import fastq_ref
import oracle
from fastq_ref import CASES, MALFORMED, fastq_to_fasta
from gpu_support import check_fastq_against_oracle, count_fastq, env_without_ranks, lib, record_names, run_py

pytestmark = pytest.mark.gpu


def _adversarial() -> bytes:
    """Every hand-written case that stands alone in one stream (cases without a final newline go last)."""
    parts = [fq for name, fq, _ in CASES if fq and fq.endswith((b"\n", b"\r")) and name != "trailing_blank_lines" and name != "only_blank_lines"]
    fq = b"".join(parts)
    return fq + b"@last\r\nACGTTTGACCA\r\n+\r\n@>+ACGTIIII"


@pytest.mark.parametrize("k", [3, 7, 15])
def test_adversarial_cases(gpu, k):
    fq = _adversarial()
    check_fastq_against_oracle(count_fastq(fq, k), fq, k)


@pytest.mark.parametrize("name,fq,fa", CASES, ids=[c[0] for c in CASES])
def test_each_case_alone(gpu, name, fq, fa):
    got = count_fastq(fq, 7)
    assert got["stats"]["bytes_emitted"] == len(fa)
    check_fastq_against_oracle(got, fq, 7)


def test_k17_matches_fasta_path(gpu):
    """k = 17 (a 16 GiB table): the FASTQ path and the FASTA path on the converted text agree byte for byte."""
    lib = gs.lib()
    fq, fa = fastq_ref.read_set(20_000, length=150, seed=17, genome_bp=200_000)
    fq = _adversarial() + b"\r\n" + fq
    fa = fastq_to_fasta(fq)
    k, step = 17, 1 << 30
    with lib.Indexer(k, fmt="fastq") as a, lib.Indexer(k) as b:
        a.feed(fq)
        b.feed(fa)
        fa_, fb_ = a.finish(), b.finish()
        for key in ("num_kmers", "total_bp", "n_records"):
            assert fa_[key] == fb_[key], key
        assert np.array_equal(fa_["hist256"], fb_["hist256"])
        assert record_names(fq, a.records(fa_["n_records"])) == record_names(fa, b.records(fb_["n_records"]))
        ta, tb = np.empty(step, dtype=np.uint8), np.empty(step, dtype=np.uint8)
        for off in range(0, 4 ** k, step):
            a.table_slice_to_host(ta, off)
            b.table_slice_to_host(tb, off)
            assert np.array_equal(ta, tb), off
    want = oracle.kmer_list(fa, k)
    assert fa_["num_kmers"] == want.size


def test_long_single_line_read(gpu):
    """A 2.5 Mbp read on one line spans 150 chunks; fed in pieces that cut it (and its quality) anywhere."""
    rng = np.random.default_rng(5)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 2_500_000)]
    seq[rng.random(seq.size) < 0.001] = ord("N")
    fq = b"@long read\n" + seq.tobytes() + b"\n+\n" + bytes(rng.integers(33, 74, seq.size, dtype=np.uint8)) + b"\n"
    fq += b"@short\nACGTACGTAAAC\n+\nIIIIIIIIIIII\n"
    for cuts in (None, [7, 1 << 20, (1 << 20) + 1, 2_500_020, 2_500_021, 4_000_000]):
        check_fastq_against_oracle(count_fastq(fq, 15, cuts=cuts), fq, 15)


def test_million_short_reads_grow_the_record_array(gpu):
    fq, fa = fastq_ref.read_set(1_100_000, length=24, seed=11, genome_bp=1 << 16, n_rate=0.01)
    got = count_fastq(fq, 7)
    want = oracle.count_fasta(fa, 7)
    assert got["num_kmers"] == want["num_kmers"] and got["total_bp"] == want["total_bp"]
    assert np.array_equal(got["table"], want["table"])
    assert got["n_records"] == 1_100_000 == len(want["records"])
    assert np.array_equal(got["records"]["seq_len"], want["records"]["seq_len"])
    assert np.array_equal(got["records"]["n_valid_kmers"], want["records"]["n_valid_kmers"])
    assert np.array_equal(got["records"]["name_len"], want["records"]["name_len"])
    i = np.array([0, 1, 777, 500_000, 1_099_999])
    assert record_names(fq, got["records"][i]) == record_names(fa, want["records"][i])
    assert got["stats"] == {"records": 1_100_000, "lines": 4_400_000, "bytes_fed": len(fq), "bytes_emitted": len(fa)}


def _cuts(fq: bytes, rng, n_small: int):
    """Random cuts from 1 byte to MBs, plus cuts inside every kind of place: a "\\r\\n" pair, a name, between lines 3 and 4."""
    cuts = set()
    crlf = [i + 1 for i in range(0, min(len(fq), 4000)) if fq[i:i + 2] == b"\r\n"][:20]
    cuts.update(crlf)
    at = [i for i in range(min(len(fq), 4000)) if fq[i] == ord("@")][:20]
    cuts.update(a + 2 for a in at)
    lines = fastq_ref.lines(fq[:200_000])
    cuts.update(lines[j][0] for j in range(3, min(len(lines), 200), 4))          # line 4 starts: between lines 3 and 4
    pos = 0
    while pos < len(fq):
        pos += int(rng.choice([1, 2, 3, 15, 64, 1000, 16384, 100_000, 3_000_000]))
        cuts.add(pos)
    cuts.update(int(x) for x in rng.integers(0, len(fq), n_small))
    return sorted(c for c in cuts if 0 < c < len(fq))


@pytest.mark.parametrize("crlf", [False, True])
def test_random_cuts_give_identical_results(gpu, crlf):
    rng = np.random.default_rng(21 + crlf)
    fq, _ = fastq_ref.read_set(40_000, length=150, seed=4 + crlf, genome_bp=1 << 18, crlf=crlf)
    fq = _adversarial() + b"\r\n" + fq
    whole = count_fastq(fq, 15)
    check_fastq_against_oracle(whole, fq, 15)
    cut = count_fastq(fq, 15, cuts=_cuts(fq, rng, 100))
    for key in ("num_kmers", "total_bp", "n_records", "stats"):
        assert cut[key] == whole[key], key
    assert np.array_equal(cut["table"], whole["table"]) and np.array_equal(cut["hist256"], whole["hist256"])
    assert np.array_equal(cut["records"], whole["records"])


def test_read_set_200mbp_matches_gpu_fasta_path(gpu):
    """~200 Mbp of 150 bp reads at k = 15 through feed_device: the FASTQ table is byte-identical to the FASTA path's."""
    lib = gs.lib()
    fq, fa = fastq_ref.read_set(1_350_000, length=150, seed=9, genome_bp=50_000_000)
    tables, fins = [], []
    for data, fmt in ((fq, "fastq"), (fa, "fasta")):
        buf = lib.DeviceBuffer(len(data))
        buf.upload(np.frombuffer(data, dtype=np.uint8))
        with lib.Indexer(15, fmt=fmt) as ix:
            ix.feed_device(buf.ptr, len(data))
            fins.append(ix.finish())
            fins[-1]["records"] = ix.records(fins[-1]["n_records"])
            tables.append(ix.table_to_host())
            if fmt == "fastq":
                assert ix.fastq_stats()["bytes_emitted"] == len(fa)
        buf.free()
    assert np.array_equal(tables[0], tables[1])
    for key in ("num_kmers", "total_bp", "n_records"):
        assert fins[0][key] == fins[1][key]
    assert np.array_equal(fins[0]["hist256"], fins[1]["hist256"])
    for f in ("name_len", "seq_len", "n_valid_kmers"):
        assert np.array_equal(fins[0]["records"][f], fins[1]["records"][f])
    i = np.array([0, 12345, 1_349_999])
    assert record_names(fq, fins[0]["records"][i]) == record_names(fa, fins[1]["records"][i])


def test_address_slices_concatenate(gpu):
    fq, _ = fastq_ref.read_set(30_000, length=150, seed=8, genome_bp=1 << 18)
    fq = _adversarial() + b"\r\n" + fq
    whole = count_fastq(fq, 15)
    parts = [count_fastq(fq, 15, n_slices=4, slice_index=s) for s in range(4)]
    assert np.array_equal(np.concatenate([p["table"] for p in parts]), whole["table"])
    assert sum(p["hist256"][1:].sum() for p in parts) == whole["hist256"][1:].sum()
    for p in parts:
        assert p["num_kmers"] == whole["num_kmers"] and np.array_equal(p["records"], whole["records"])


@pytest.mark.parametrize("name,fq,rec,rule", MALFORMED, ids=[c[0] for c in MALFORMED])
def test_malformed_then_reset(gpu, name, fq, rec, rule):
    lib = gs.lib()
    good, _ = fastq_ref.read_set(300, length=60, seed=2, genome_bp=5000)
    for cuts in (None, list(range(1, len(fq)))):                    # whole, and one byte per feed
        with lib.Indexer(7, fmt="fastq") as ix:
            with pytest.raises(lib.PkError) as e:
                if cuts is None:
                    ix.feed(fq)
                else:
                    for i in range(len(fq)):
                        ix.feed(fq[i:i + 1])
                ix.finish()
            assert e.value.code == lib.PK_ERR_FORMAT
            want = fastq_ref.FastqError(rec, [s for s, _, _ in fastq_ref.lines(fq)][4 * (rec - 1)], rule)
            assert str(want) in str(e.value), (str(e.value), str(want))
            with pytest.raises(lib.PkError) as again:                 # it stays stopped until a reset
                ix.feed(good)
            assert again.value.code == lib.PK_ERR_FORMAT
            ix.reset()
            ix.feed(good)
            fin = ix.finish()
            fin["records"], fin["stats"], fin["table"] = ix.records(fin["n_records"]), ix.fastq_stats(), ix.table_to_host()
            check_fastq_against_oracle(fin, good, 7)


def test_format_is_set_before_the_first_feed(gpu):
    lib = gs.lib()
    fq, _ = fastq_ref.read_set(10, length=30, seed=1, genome_bp=1000)
    with lib.Indexer(7) as ix:
        ix.feed(fq[:0])
        lib._check(lib.load().pk_indexer_set_format(ix._h, lib.PK_FORMAT_FASTQ))
        ix.feed(fq)
        rc = lib.load().pk_indexer_set_format(ix._h, lib.PK_FORMAT_FASTA)
        assert rc == lib.PK_ERR_STATE
        ix.finish()
        ix.reset()                                                   # the format stays
        ix.feed(fq)
        assert ix.fastq_stats()["records"] == 10
    with lib.Indexer(7) as ix:
        assert lib.load().pk_indexer_set_format(ix._h, 7) == lib.PK_ERR_ARG


def test_indexer_cli_fastq_plain_gz_bgz(gpu, tmp_path):
    from pykmer_amd import bgzf
    fq, fa = fastq_ref.read_set(5000, length=100, seed=6, genome_bp=100_000)
    fq = _adversarial() + b"\r\n" + fq
    fa = fastq_to_fasta(fq)
    (tmp_path / "reads.fa").write_bytes(fa)
    (tmp_path / "reads.fq").write_bytes(fq)
    with gzip.open(tmp_path / "reads.fq.gz", "wb") as fh:
        fh.write(fq)
    bgzf.compress_file(str(tmp_path / "reads.fq"), str(tmp_path / "reads.fq.bgz"))
    assert bgzf.is_bgzf(str(tmp_path / "reads.fq.bgz"))
    out = run_py("indexer.py", str(tmp_path / "reads.fa"), "s", "9", cwd=str(tmp_path), timeout=900).stdout
    assert "READING FASTA FROM" in out
    with open(tmp_path / "reads.fa.09.kin.json") as fh:
        want = json.load(fh)
    kin_fa = (tmp_path / "reads.fa.09.kin").read_bytes()
    for name in ("reads.fq", "reads.fq.gz", "reads.fq.bgz"):
        out = run_py("indexer.py", str(tmp_path / name), "s", "9", cwd=str(tmp_path), timeout=900).stdout
        assert "READING FASTQ FROM" in out and "READING FASTA" not in out
        with open(tmp_path / f"{name}.09.kin.json") as fh:
            got = json.load(fh)
        assert sorted(got) == sorted(want)                            # same schema, no new key
        for key in fastq_ref.DETERMINISTIC:
            assert got[key] == want[key], (name, key)
        assert (tmp_path / f"{name}.09.kin").read_bytes() == kin_fa
        assert len(got["chromosomes"]) == len(want["chromosomes"]) > 5000


def test_merger_kwip_over_fastq_tables(gpu, tmp_path):
    """Three read sets of one genome (k = 11: partly shared k-mers, so the kernel is not degenerate)."""
    genome = np.random.default_rng(30).integers(0, 4, 200_000, dtype=np.uint8)
    kins = []
    for i in range(3):
        fq, _ = fastq_ref.read_set(1000 + 500 * i, length=150, seed=30 + i, genome=genome)
        p = tmp_path / f"s{i}.fastq"
        p.write_bytes(fq)
        run_py("indexer.py", str(p), f"s{i}", "11", cwd=str(tmp_path), timeout=900)
        kins.append(f"{p}.11.kin")
    run_py("merger.py", str(tmp_path / "kw"), *kins, "--kwip", cwd=str(tmp_path), timeout=900, env=env_without_ranks())
    k = np.loadtxt(tmp_path / "kw.kern", skiprows=1, usecols=range(1, 4))
    d = np.loadtxt(tmp_path / "kw.dist", skiprows=1, usecols=range(1, 4))
    assert k.shape == d.shape == (3, 3) and np.all(np.isfinite(k)) and np.all(np.isfinite(d)) and np.allclose(d, d.T)
    assert np.all(k > 0) and np.all(np.diag(d) == 0) and np.all(d[~np.eye(3, dtype=bool)] > 0)
    from merge_ref import direct_kernel
    from pykmer_amd import merger
    tabs = [merger.Header(x, index_file=x).read_table_slice(0, 4 ** 11) for x in sorted(kins)]
    assert np.allclose(k, direct_kernel(tabs), rtol=1e-12, atol=0)


def _padded_reads(n_fasta_bytes: int, n_reads: int, length: int, seed: int):
    """(fastq, fasta): n_reads random reads of `length` bp whose FASTA text is exactly n_fasta_bytes long (the names are
    padded to make up the difference)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    name_bytes = n_fasta_bytes - n_reads * (length + 3)                     # '>' + name + '\n' + sequence + '\n'
    q, r = divmod(name_bytes, n_reads)
    assert q >= 12
    seqs = acgt[rng.integers(0, 4, (n_reads, length))]
    qual = b"I" * length
    fq, fa = [], []
    for i in range(n_reads):
        name = (b"read%d_" % i).ljust(q + (i < r), b"p")
        s = seqs[i].tobytes()
        fq.append(b"@" + name + b"\n" + s + b"\n+\n" + qual + b"\n")
        fa.append(b">" + name + b"\n" + s + b"\n")
    fa = b"".join(fa)
    assert len(fa) == n_fasta_bytes
    return b"".join(fq), fa


def test_record_overflow_after_a_relayout_feed(gpu):
    """FASTQ form of test_gpu_indexer.py's test of the same name: a long read on one line whose FASTA text defeats the bucket
    sample, then short reads whose FASTA text has the same length and far more records than the array holds.  FASTQ
    text is counted one call late: the first text's relayout happens in the second feed call, the second text's record
    retry inside finish."""
    import inputs
    from inputs import record_overflows, record_starts
    k = 15
    fa1 = inputs.skewed_fasta(20_000_000, 61, seed=72, width=None)
    head, seq = fa1.split(b"\n")[:2]
    fq1 = b"@" + head[1:] + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n"
    assert fastq_to_fasta(fq1) == fa1
    fq2, fa2 = _padded_reads(len(fa1), 120_000, 100, seed=73)
    fq, fa = fq1 + fq2, fa1 + fa2
    with lib().Indexer(k, fmt="fastq") as ix:
        ix.feed(fq1)
        ix.feed(fq2)
        assert ix.timings()["relayouts"] >= 1, "the long read was meant to overflow the sampled layout"
        fin = ix.finish()
        got = dict(fin, records=ix.records(fin["n_records"]), stats=ix.fastq_stats(), table=ix.table_to_host())
    want = oracle.count_fasta(fa, k)
    assert record_overflows([len(fa1), len(fa2)], record_starts(want["records"])) == [False, True]
    assert got["num_kmers"] == want["num_kmers"] and got["total_bp"] == want["total_bp"]
    assert got["n_records"] == len(want["records"]) == 120_001
    for f in ("name_len", "seq_len", "n_valid_kmers"):
        assert np.array_equal(got["records"][f], want["records"][f]), f
    assert record_names(fq, got["records"]) == record_names(fa, want["records"])        # name_off: the same names, sliced from the FASTQ
    assert np.array_equal(got["hist256"][1:], oracle.table_stats(want["table"])[0])
    assert np.array_equal(got["table"], want["table"])
    assert got["stats"] == fastq_ref.stats(fq)
