"""FASTQ input without a GPU: the restatement of the rules (fastq_ref), format detection by file name, the new C-ABI."""
import os
import re

import pytest

import fastq_ref
from fastq_ref import CASES, MALFORMED, FastqError, fastq_to_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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
