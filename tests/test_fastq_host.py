"""FASTQ input without a GPU: the restatement of the rules (fastq_ref), format detection by file name, the new C-ABI."""
import os
import re

import pytest

import fastq_ref
from fastq_ref import FastqError, fastq_to_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, FASTQ, the FASTA text it stands for)
CASES = [
    ("plain", b"@r1 first\nACGTACGTAC\n+\nIIIIIIIIII\n@r2\nGGGTTT\n+r2\n!!!!!!\n",
     b">r1 first\nACGTACGTAC\n>r2\nGGGTTT\n"),
    ("crlf", b"@r1\r\nACGTTGCA\r\n+\r\nIIIIIIII\r\n@r2\r\nTTTT\r\n+\r\nIIII\r\n", b">r1\r\nACGTTGCA\r\n>r2\r\nTTTT\r\n"),
    ("lone_cr", b"@r1\rACGTTGCA\r+\rIIIIIIII\r@r2\rAC\r+\rII", b">r1\rACGTTGCA\r>r2\rAC\r"),
    ("mixed_terminators", b"@a\r\nACGT\n+\rIIII\r\n@b\rCC\r\n+\nII\n", b">a\r\nACGT\n>b\rCC\r\n"),
    ("empty_reads", b"@e1\n\n+\n\n@r\nACG\n+\nIII\n@e2\n\n+\n\n", b">e1\n\n>r\nACG\n>e2\n\n"),
    ("quality_starts_with_at_plus_gt", b"@r1\nACGT\n+\n@III\n@r2\nACGT\n+\n+III\n@r3\nACGT\n+\n>III\n",
     b">r1\nACGT\n>r2\nACGT\n>r3\nACGT\n"),
    ("quality_all_acgt", b"@q\nACGTACGT\n+\nACGTACGT\n@q2\nTTTT\n+q2\nGGGG\n", b">q\nACGTACGT\n>q2\nTTTT\n"),
    ("no_final_newline", b"@r1\nACGTA\n+\nIIIII\n@r2\nCCCC\n+\nIIII", b">r1\nACGTA\n>r2\nCCCC\n"),
    ("trailing_blank_lines", b"@r1\nACGTA\n+\nIIIII\n\n\n\r\n\r\n\n\n\n", b">r1\nACGTA\n"),
    ("name_with_blanks_and_tabs", b"@r1 a\tb  \nAC GT\n+\nIIIII\n", b">r1 a\tb  \nAC GT\n"),
    ("lower_case_and_n", b"@x\nacgtNNacgt\n+\nIIIIIIIIII\n", b">x\nacgtNNacgt\n"),
    ("seq_with_leading_blank", b"@x\n  ACGT\n+\nIIIIII\n", b">x\n  ACGT\n"),
    ("empty_stream", b"", b""),
    ("only_blank_lines", b"\n\n\r\n", b""),
]

# (name, FASTQ, 1-based record, rule)
MALFORMED = [
    ("no_at", b"@r1\nAC\n+\nII\nr2\nAC\n+\nII\n", 2, 1),
    ("fasta_given_as_fastq", b">r1\nACGT\nACGT\n>r2\nAC\n", 1, 1),
    ("seq_begins_with_gt", b"@r1\nAC\n+\nII\n@r2\n>AC\n+\nIII\n", 2, 2),
    ("seq_begins_with_gt_after_blanks", b"@r1\n \t>AC\n+\nIIIII\n", 1, 2),
    ("no_plus", b"@r1\nAC\n+\nII\n@r2\nAC\n-\nII\n", 2, 3),
    ("empty_line_3", b"@r1\nAC\n\nII\n", 1, 3),
    ("quality_too_short", b"@r1\nACGT\n+\nIII\n@r2\nAC\n+\nII\n", 1, 4),
    ("quality_too_long_last", b"@r1\nAC\n+\nII\n@r2\nACGT\n+\nIIIII", 2, 4),
    ("wrapped", b"@r1\nACGT\nACGT\n+\nIIII\nIIII\n", 1, 3),
    ("ends_after_line_2", b"@r1\nAC\n+\nII\n@r2\nACGT\n", 2, 5),
    ("ends_inside_line_1", b"@r1\nAC\n+\nII\n@r2", 2, 5),
    ("ends_before_line_4", b"@r1\nAC\n+\nII\n@r2\n\n+\n", 2, 5),
    ("blank_line_then_record", b"@r1\nAC\n+\nII\n\n@r2\nAC\n+\nII\n", 2, 1),
    ("text_after_blank_lines", b"@r1\nAC\n+\nII\n\n\n\nx", 2, 1),
]


@pytest.mark.parametrize("name,fq,fa", CASES, ids=[c[0] for c in CASES])
def test_restatement_cases(name, fq, fa):
    assert fastq_to_fasta(fq) == fa


def test_restatement_cr_lf_cut_and_roles():
    # a "\r\n" pair is one terminator wherever a feed cuts it; roles come from line numbers, never from content
    fq = b"@r\r\nAC\r\n+\r\n@>\r\n"
    assert fastq_to_fasta(fq) == b">r\r\nAC\r\n"
    assert fastq_ref.lines(fq)[0] == (0, 2, 4)
    assert fastq_ref.stats(fq) == {"records": 1, "lines": 4, "bytes_fed": len(fq), "bytes_emitted": 8}
    assert fastq_ref.stats(b"@r\nA\n+\nI\n\n\n") == {"records": 1, "lines": 6, "bytes_fed": 11, "bytes_emitted": 5}


@pytest.mark.parametrize("name,fq,rec,rule", MALFORMED, ids=[c[0] for c in MALFORMED])
def test_restatement_malformed(name, fq, rec, rule):
    with pytest.raises(FastqError) as e:
        fastq_to_fasta(fq)
    assert (e.value.record, e.value.rule) == (rec, rule)
    starts = [s for s, _, _ in fastq_ref.lines(fq)]
    assert e.value.offset == starts[4 * (rec - 1)]


def test_read_set_generator_matches_restatement():
    for crlf in (False, True):
        fq, fa = fastq_ref.read_set(500, length=150, seed=3, genome_bp=10_000, crlf=crlf)
        assert fastq_to_fasta(fq) == fa
        assert fastq_ref.stats(fq)["records"] == 500


def test_format_from_file_name():
    from pykmer_amd.indexer import input_format
    for n in ("reads.fq", "reads.fastq", "a/b.fq.gz", "x.fastq.gz", "x.fq.bgz", "x.fastq.bgz"):
        assert input_format(n) == "fastq", n
    for n in ("g.fa", "g.fa.gz", "g.fasta", "g.fa.bgz", "fq", "reads.fq.txt", "reads.fqgz", "reads.FQ", "x.fastq.zip", "fq.fa"):
        assert input_format(n) == "fasta", n


def test_new_symbols_declared_and_bound():
    from pykmer_amd import _lib
    header = open(os.path.join(ROOT, "include", "pykmer_hip.h")).read()
    for name in ("pk_indexer_set_format", "pk_indexer_fastq_stats"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.EXPORTS
    assert re.search(r"PK_ERR_FORMAT = -5", header) and _lib.PK_ERR_FORMAT == -5
    assert "#define PK_FORMAT_FASTA 0" in header and "#define PK_FORMAT_FASTQ 1" in header
    assert (_lib.PK_FORMAT_FASTA, _lib.PK_FORMAT_FASTQ) == (0, 1)
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert hasattr(lib, "pk_indexer_set_format") and hasattr(lib, "pk_indexer_fastq_stats")
    with pytest.raises(ValueError):
        _lib.Indexer(7, fmt="sam")
