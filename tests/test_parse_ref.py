"""CPU: the bytes-level parser twin (parse_ref) against pyoracle on ASCII and against the C oracle on every byte value,
and the route conditions of the generators in byte_inputs (they assert them themselves when called)."""
import numpy as np
import pytest

import byte_inputs
import inputs
import oracle
import parse_ref
from fastq_ref import fastq_to_fasta
from oracle import pyoracle

FIELDS = ("name_off", "name_len", "seq_len", "n_valid_kmers")


def _twin_equals_c_oracle(data: bytes, k: int):
    recs, kmers = parse_ref.parse(data, k)
    want_kmers, want = oracle.kmer_list(data, k, records=True)
    assert len(recs) == len(want["records"])
    for f in FIELDS:
        assert np.array_equal(recs[f], want["records"][f]), (k, f)
    assert np.array_equal(kmers, want_kmers), k
    assert int(recs["seq_len"].sum()) == want["total_bp"] and kmers.size == want["num_kmers"]
    return recs


@pytest.mark.parametrize("k", [1, 5, 9])
def test_twin_equals_pyoracle_on_ascii(k):
    """The anchor: on an ASCII text the twin is pyoracle, which the goldens pin to the reference."""
    data = inputs.edge_fasta()
    recs, kmers = parse_ref.parse(data, k)
    _, num_kmers, _, everything = pyoracle.count_fasta(data, k)
    assert [n.decode("ascii") for n in parse_ref.names(data, recs)] == [name for name, _, _ in everything]
    assert recs["seq_len"].tolist() == [s for _, s, _ in everything]
    assert recs["n_valid_kmers"].tolist() == [v for _, _, v in everything]
    want = [min(fwd, rev) for _, seq, _ in pyoracle.records(data.decode("ascii")) for _, fwd, rev in pyoracle.windows(seq, k)]
    assert kmers.tolist() == want and len(want) == num_kmers
    _twin_equals_c_oracle(data, k)


def test_c_oracle_equals_twin_on_placement_texts():
    for dense in (False, True):
        for text in byte_inputs.placement_fasta(dense):
            for k in (3, 15):
                _twin_equals_c_oracle(text, k)


def test_c_oracle_equals_twin_on_line_starts_and_headers():
    text = byte_inputs.line_start_fasta()
    recs = _twin_equals_c_oracle(text, 5)
    # 256 '>vNNN' records, the leading one, and the three lines that begin with '>' itself: no near miss opened a record
    assert len(recs) == 1 + 256 + 3
    for t in byte_inputs.stream_start_fastas():
        recs = _twin_equals_c_oracle(t, 5)
        assert len(recs) == (2 if t[:1] == b">" else 1)
    text = byte_inputs.header_bytes_fasta()
    recs = _twin_equals_c_oracle(text, 5)
    names = parse_ref.names(text, recs)
    assert any(n.endswith(b"\xa0\xa0") and len(n) == 130 for n in names) and any(len(n) == 70 for n in names)
    across = [r for r in recs if int(r["name_off"]) < byte_inputs.CHUNK < int(r["name_off"]) + int(r["name_len"])]
    assert len(across) == 1                                   # one name lies across the 16 KiB seam
    small = byte_inputs.header_bytes_fasta(byte_inputs.CLI_NAME_VALUES)
    assert 45 <= len(_twin_equals_c_oracle(small, 5)) <= 60


def test_c_oracle_equals_twin_on_soups():
    for seed, n in byte_inputs.SOUP_CASES:
        data = byte_inputs.soup(seed, n)
        for k in (3, 9):
            _twin_equals_c_oracle(data, k)
    first = byte_inputs.soup(*byte_inputs.SOUP_CASES[0])
    for m in byte_inputs.SOUP_PREFIXES:
        _twin_equals_c_oracle(first[:m], 3)
    cuts = byte_inputs.cuts_around_odd_bytes(first, seed=5)
    a = np.frombuffer(first, dtype=np.uint8)
    ones = [c for c, d in zip(cuts[:-1], cuts[1:]) if d == c + 1]
    assert len(ones) >= 50 and (a[ones] >= 0x80).sum() >= 25 and (a[ones] < 0x21).sum() >= 25


@pytest.mark.parametrize("crlf", [False, True])
def test_c_oracle_equals_twin_on_fastq_placements(crlf):
    fq = byte_inputs.placement_fastq(crlf)
    fa = fastq_to_fasta(fq)
    recs = _twin_equals_c_oracle(fa, 3)
    assert len(recs) == 254 * 5 + (254 - 8 - 1)              # six records per value; the last kind not for blanks and '>'
    _twin_equals_c_oracle(fa, 15)


def test_bytes_that_python_would_strip_after_a_decode_are_not_blanks():
    """str.strip() strips U+0085 (NEL) and U+00A0 (NBSP), which a Latin-1 decode makes of the bytes 0x85 and 0xA0 and a
    UTF-8 decode of 0xC2 0x85 and 0xC2 0xA0.  The project's rule is on bytes: only the ten ASCII blanks are
    blanks, so each of these bytes is one invalid sequence character, is kept at either end of a line and of a name, and
    never makes a line empty."""
    assert "\x85\xa0".strip() == "" and b"\xc2\x85\xc2\xa0".decode("utf-8").strip() == ""   # what Python would do
    for odd in (b"\x85", b"\xa0", b"\xc2\x85", b"\xc2\xa0"):
        n = len(odd)
        text = b">name" + odd + b"\n" + odd + b"ACGTA" + odd + b"\n" + odd + b"\nACG" + odd + b"TTGCA\n" + odd + b">not a header\n"
        for use in (oracle.count_fasta, lambda d, k: {"records": parse_ref.parse(d, k)[0]}):
            recs = use(text, 3)["records"]
            assert len(recs) == 1                             # odd + '>' at a line start opens no record
            r = recs[0]
            assert int(r["name_len"]) == 4 + n                # kept at the end of the name
            assert int(r["seq_len"]) == (n + 5 + n) + n + (3 + n + 5) + (n + len(b">not a header"))
            assert int(r["n_valid_kmers"]) == 3 + 1 + 3       # ACGTA; ACG; TTGCA: the odd bytes cut every window
        assert oracle.count_fasta(text, 3)["num_kmers"] == 7
