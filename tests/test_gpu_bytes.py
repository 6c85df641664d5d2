"""GPU: all 256 byte values through the FASTA, FASTQ and query parsers, bit-exact against the C oracle.

The structure pass, the squeeze pass and the FASTQ front end classify text four bytes at a time (swar_zero / swar_less, a
v_perm_b32 table keyed on byte & 7, movemask4 on bit 7); bit 7 of the INPUT byte is where such code goes wrong.  The texts
come from byte_inputs, whose generators assert the route each text takes; tests/test_parse_ref.py pins the oracle's
reading of these bytes to the bytes-level twin of pyoracle (parse_ref)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import byte_inputs
import oracle
import parse_ref
import query_ref
from gpu_support import Device, check_against_oracle, check_fastq_against_oracle, count_fastq, query, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("name_off", "name_len", "seq_len", "n_valid_kmers")


@pytest.mark.parametrize("dense", [False, True])
def test_every_byte_value_at_piece_and_chunk_edges(gpu, dense):
    """k = 3 keeps windows alive between foreign bytes; k = 15 is the literal instantiation, 14 carried bases at a seam."""
    for text in byte_inputs.placement_fasta(dense):
        for k in (3, 15):
            check_against_oracle(gpu, text, k)


def test_every_byte_value_at_line_starts(gpu):
    text = byte_inputs.line_start_fasta()
    got = check_against_oracle(gpu, text, 5)
    assert len(got["records"]) == 1 + 256 + 3                 # only '>' opened records: not 0xBE, 0x1E, 0x3C, 0x3F, 0x7E
    for t in byte_inputs.stream_start_fastas():
        check_against_oracle(gpu, t, 5)


def test_every_byte_value_in_header_text(gpu):
    text = byte_inputs.header_bytes_fasta()
    got = check_against_oracle(gpu, text, 5)
    want, _ = parse_ref.parse(text, 5)
    assert parse_ref.names(text, got["records"]) == parse_ref.names(text, want)


def _streamed(gpu, data: bytes, k: int, cuts):
    with gpu.Indexer(k) as ix:
        for a, b in zip(cuts[:-1], cuts[1:]):
            ix.feed(data[a:b])
        fin = ix.finish()
        fin["records"] = ix.records(fin["n_records"])
        fin["table"] = ix.table_to_host()
    return fin


def test_full_alphabet_soup(gpu):
    for seed, n in byte_inputs.SOUP_CASES:
        data = byte_inputs.soup(seed, n)
        for k in (3, 9):
            check_against_oracle(gpu, data, k)
    first = byte_inputs.soup(*byte_inputs.SOUP_CASES[0])
    for m in byte_inputs.SOUP_PREFIXES:
        check_against_oracle(gpu, first[:m], 3)
    # the same bytes through the streaming interface: cuts immediately before and behind bytes >= 0x80 and bytes < 0x21,
    # each of those also as a feed of one byte
    cuts = byte_inputs.cuts_around_odd_bytes(first, seed=5)
    for k in (3, 9):
        whole = check_against_oracle(gpu, first, k)
        want = oracle.count_fasta(first, k)
        fin = _streamed(gpu, first, k, cuts)
        assert fin["num_kmers"] == want["num_kmers"] == whole["num_kmers"] and fin["total_bp"] == want["total_bp"]
        assert fin["n_records"] == len(want["records"])
        for f in FIELDS:
            assert np.array_equal(fin["records"][f], want["records"][f]), (k, f)
            assert np.array_equal(fin["records"][f], whole["records"][f]), (k, f)
        assert np.array_equal(fin["table"], want["table"]) and np.array_equal(fin["table"], whole["table"])
        assert np.array_equal(fin["hist256"], whole["hist256"])
        assert np.array_equal(fin["hist256"][1:], oracle.table_stats(want["table"])[0])


@pytest.mark.parametrize("crlf", [False, True])
def test_fastq_every_byte_value_in_every_line_role(gpu, crlf):
    fq = byte_inputs.placement_fastq(crlf)
    for k in (3, 15):
        check_fastq_against_oracle(count_fastq(fq, k), fq, k)
    rng = np.random.default_rng(40 + crlf)
    cuts = sorted(set(int(c) for c in rng.integers(1, len(fq), size=40)))
    check_fastq_against_oracle(count_fastq(fq, 3, cuts=cuts), fq, 3)


def test_query_over_full_alphabet_text(gpu):
    k = 9
    tables = query_ref.random_tables(k, 2, seed=61)
    texts = [byte_inputs.soup(*byte_inputs.SOUP_CASES[0]), *byte_inputs.placement_fasta(False)]   # all three placement texts
    with Device(tables) as dev:
        for text in texts:
            want = query_ref.expected(text, k, tables, 1, 255)
            assert want["hits"].any(axis=0).all() and int(want["n_valid"].sum()) >= 500   # not a vacuous comparison
            same(query(text, k, dev.ptrs, 1, 255), want)


def test_cli_names_that_are_not_utf8(gpu, tmp_path):
    """Header names are byte ranges; the CLI shows them as utf-8 with 'replace' (pykmer_amd/indexer.py, count_file).  Names
    with NUL, a quote-worthy backslash, lone continuation bytes, truncated multi-byte sequences and 0xFF must give a
    .kin.json that loads, not a crash."""
    k = 7
    text = byte_inputs.header_bytes_fasta(byte_inputs.CLI_NAME_VALUES)
    fa = tmp_path / "names.fa"
    fa.write_bytes(text)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "indexer.py"), str(fa), "names", str(k)], cwd=str(tmp_path),
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(f"{fa}.{k:02d}.kin.json") as fh:
        meta = json.load(fh)
    want = oracle.count_fasta(text, k)
    listed = [r for r in want["records"] if r["n_valid_kmers"]]
    assert 45 <= len(listed) <= 60
    raw = parse_ref.names(text, listed)
    assert any(b"\xff" in n for n in raw) and any(b"\x00" in n for n in raw)
    assert [c[1] for c in meta["chromosomes"]] == [int(r["seq_len"]) for r in listed]
    assert [c[0] for c in meta["chromosomes"]] == [n.decode("utf-8", "replace") for n in raw]
    assert meta["num_kmers"] == want["num_kmers"]
