"""Base qualities without a GPU: the restatement of the rule (fastq_qual_ref), the new C-ABI, the CLIs' argument errors."""
import os
import re

import pytest

import fastq_ref
from fastq_qual_ref import biased_qualities, hand_qualities, mask_fastq_to_fasta
from fastq_ref import CASES, MALFORMED, fastq_to_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WELL_FORMED = [fq for _, fq, _ in CASES]


def _min_quality(fq: bytes) -> int:
    ls = fastq_ref.lines(fq)
    quals = [fq[s:e] for s, e, _ in ls[3::4]]
    return min((min(q) for q in quals if q), default=255)


@pytest.mark.parametrize("name,fq,fa", CASES, ids=[c[0] for c in CASES])
def test_off_and_thresholds_up_to_the_smallest_quality(name, fq, fa):
    assert mask_fastq_to_fasta(fq, 0) == (fa, 0)
    lowest = _min_quality(fq)
    for T in (1, lowest):
        assert mask_fastq_to_fasta(fq, T) == (fastq_to_fasta(fq), 0), T


@pytest.mark.parametrize("T", [1, 34, 53, 128, 200, 255])
def test_length_does_not_depend_on_the_threshold(T):
    for i, fq in enumerate(WELL_FORMED):
        fq = hand_qualities(fq, T, seed=i)
        fa, n = mask_fastq_to_fasta(fq, T)
        plain = fastq_to_fasta(fq)
        assert len(fa) == len(plain)
        assert n >= sum(a != b for a, b in zip(fa, plain))           # a low-quality N is counted and looks the same
        assert all(a == b or a == ord("N") for a, b in zip(fa, plain))
        assert fastq_ref.lines(fa) == fastq_ref.lines(plain)          # the same lines: no terminator was touched


def test_blanks_are_never_replaced():
    blanks = b" \t\x0b\x0c\x1c\x1d\x1e\x1f"                           # the blanks a line can hold (not its terminators)
    seq = b" \tAC" + blanks + b"GT\x1f "
    fq = b"@r\n" + seq + b"\n+\n" + b"!" * len(seq) + b"\n"
    fa, n = mask_fastq_to_fasta(fq, 34)
    assert fa == b">r\n \tNN" + blanks + b"NN\x1f \n" and n == 4
    # lone '\r' lines and "\r\n": the terminators are no line-2 bytes
    fq = b"@r\r\nA C\r\n+\r\n!!!\r\n@s\rG\tT\r+\r!!!"
    assert mask_fastq_to_fasta(fq, 255) == (b">r\r\nN N\r\n>s\rN\tN\r", 4)


def test_the_threshold_is_exclusive_and_unsigned():
    for T in (1, 2, 34, 53, 97, 128, 129, 255):
        qual = bytes([T - 1, T, T - 1, min(T + 1, 255)])
        fq = b"@r\nACGT\n+\n" + qual + b"\n"
        if 10 in qual or 13 in qual:
            continue
        assert mask_fastq_to_fasta(fq, T) == (b">r\nNCNT\n", 2), T
    # bytes >= 0x80 are large, bytes below the offset are small: no special rule
    fq = b"@r\nACGTA\n+\n\x00\x7f\x80\xff\x20\n"
    assert mask_fastq_to_fasta(fq, 33) == (b">r\nNCGTN\n", 2)
    assert mask_fastq_to_fasta(fq, 0x80) == (b">r\nNNGTN\n", 3)
    assert mask_fastq_to_fasta(fq, 0xFF) == (b">r\nNNNTN\n", 4)


def test_hand_written_records_pin_the_count():
    fq = (b"@a\nACGTACGT\n+\nIIII!!!!\n"                            # 4 low
          b"@b\nNNNN\n+\n!I!I\n"                                     # a low-quality N counts as replaced: 2
          b"@c\n\n+\n\n"                                             # an empty read
          b"@d\nAC GT\n+\n!!!!!\n"                                   # the blank stays: 4
          b"@e\nacgt\n+\n5555")                                      # no final newline; '5' = 53
    assert mask_fastq_to_fasta(fq, 34) == (b">a\nACGTNNNN\n>b\nNNNN\n>c\n\n>d\nNN NN\n>e\nacgt\n", 10)
    assert mask_fastq_to_fasta(fq, 53)[1] == 10
    assert mask_fastq_to_fasta(fq, 54) == (b">a\nACGTNNNN\n>b\nNNNN\n>c\n\n>d\nNN NN\n>e\nNNNN\n", 14)
    assert mask_fastq_to_fasta(fq, 74) == (b">a\nNNNNNNNN\n>b\nNNNN\n>c\n\n>d\nNN NN\n>e\nNNNN\n", 20)


@pytest.mark.parametrize("name,fq,rec,rule", MALFORMED, ids=[c[0] for c in MALFORMED])
def test_malformed_files_fail_as_without_masking(name, fq, rec, rule):
    with pytest.raises(fastq_ref.FastqError) as e:
        mask_fastq_to_fasta(fq, 255)
    assert (e.value.record, e.value.rule) == (rec, rule)


def test_generators_keep_the_stream_well_formed():
    fq, fa = fastq_ref.read_set(50, length=40, seed=1, genome_bp=2000)
    low = biased_qualities(fq, 53, 0.3, seed=2)
    assert len(low) == len(fq) and fastq_to_fasta(low) == fa
    masked, n = mask_fastq_to_fasta(low, 53)
    assert 0.2 * 2000 < n < 0.4 * 2000 and masked != fa and len(masked) == len(fa)
    assert mask_fastq_to_fasta(low, 43) == (fa, 0)                   # nothing lies below T - 10


def test_threshold_byte_of_the_options():
    from pykmer_amd.indexer import qual_threshold
    assert qual_threshold("r.fq", None) == 0 and qual_threshold("g.fa", None) == 0
    assert qual_threshold("r.fq", 0) == 0 and qual_threshold("r.fq", 0, 64) == 0
    assert qual_threshold("r.fq", 20) == 53 and qual_threshold("r.fastq.gz", 20, 64) == 84 and qual_threshold("r.fq.bgz", 222) == 255
    for args in (("g.fa", 20), ("g.fa.gz", 20, 33), ("r.fq", -1), ("r.fq", 223), ("r.fq", 192, 64), ("r.fq", None, 33), ("r.fq", 20, 32),
                 ("r.fq", 2.5), ("r.fq", True)):
        with pytest.raises(ValueError):
            qual_threshold(*args)


def test_new_symbols_declared_and_bound():
    from pykmer_amd import _lib
    header = open(os.path.join(ROOT, "include", "pykmer_hip.h")).read()
    for name in ("pk_indexer_set_min_qual", "pk_indexer_fastq_masked"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.EXPORTS
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert hasattr(lib, "pk_indexer_set_min_qual") and hasattr(lib, "pk_indexer_fastq_masked")
        assert lib.pk_version() == 3
    with pytest.raises(ValueError):
        _lib.Indexer(7, fmt="fasta", min_qual_byte=53)              # refused before the library is asked


INDEXER_ERRORS = [
    (["g.fa", "s", "7", "--min-qual", "20"], "FASTQ"),
    (["--min-qual", "20", "g.fa", "7"], "FASTQ"),
    (["r.fq", "s", "7", "--min-qual", "-1"], "negative"),
    (["r.fq", "--min-qual=223", "s", "7"], "255"),
    (["r.fq", "s", "--qual-offset", "64", "7", "--min-qual", "192"], "255"),
    (["r.fq", "s", "7", "--qual-offset", "64"], "--min-qual"),
    (["r.fq", "s", "7", "--min-qual", "20", "--qual-offset", "50"], "33 or 64"),
    (["r.fq", "s", "7", "--min-qual", "twenty"], "integer"),
]


@pytest.mark.parametrize("argv,word", INDEXER_ERRORS, ids=[" ".join(a) for a, _ in INDEXER_ERRORS])
def test_indexer_cli_argument_errors(argv, word, tmp_path, monkeypatch, capsys):
    from pykmer_amd import indexer
    monkeypatch.chdir(tmp_path)
    (tmp_path / "g.fa").write_bytes(b">g\nACGTACGTACGT\n")
    (tmp_path / "r.fq").write_bytes(b"@r\nACGTACGTACGT\n+\nIIIIIIIIIIII\n")
    with pytest.raises(SystemExit) as e:
        indexer.main(list(argv))
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err.startswith("error: ") and word in err
    assert sorted(p.name for p in tmp_path.iterdir()) == ["g.fa", "r.fq"]      # no file was written


QUERY_ERRORS = [
    (["--min-qual", "20"], "q.fa", "FASTQ"),
    (["--qual-offset", "64"], "q.fq", "--min-qual"),
    (["--min-qual", "-3"], "q.fq", "negative"),
    (["--min-qual", "200", "--qual-offset", "64"], "q.fq", "255"),
]


@pytest.mark.parametrize("opts,qfile,word", QUERY_ERRORS, ids=[" ".join(o) + " " + q for o, q, _ in QUERY_ERRORS])
def test_query_cli_argument_errors(opts, qfile, word, tmp_path, monkeypatch, capsys):
    from pykmer_amd import query
    monkeypatch.chdir(tmp_path)
    (tmp_path / qfile).write_bytes(b"")
    with pytest.raises(SystemExit) as e:
        query.main(["proj", qfile, "t.kin"] + list(opts))
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert err.startswith("error: ") and word in err
    assert sorted(p.name for p in tmp_path.iterdir()) == [qfile]


def test_query_json_keys_only_with_the_option():
    from pykmer_amd.query import _qual_keys
    assert _qual_keys({"hits": 1}) == {}
    assert _qual_keys({"min_qual": 20, "qual_offset": 33}) == {"min_qual": 20, "qual_offset": 33}
