"""Plain-Python restatement of the FASTQ input rules (README "FASTQ input"), for the tests only.

fastq_to_fasta(data) is the FASTA text a FASTQ stream stands for; the GPU front end (fastq.hip) must count a FASTQ
exactly as the FASTA pipeline counts this text, and emit exactly len(fastq_to_fasta(data)) bytes into it.
"""
import re
from typing import List, Tuple

import numpy as np

WS = b" \t\n\v\f\r\x1c\x1d\x1e\x1f"          # str.strip() whitespace, ASCII

RULES = {
    1: "line 1 must begin with '@'",
    2: "line 2 must not begin with '>'",
    3: "line 3 must begin with '+'",
    4: "line 4 must be as long as line 2",
    5: "the stream ends inside the record",
}


class FastqError(ValueError):
    def __init__(self, record: int, offset: int, rule: int):
        super().__init__(f"record {record} (line 1 at byte {offset}): {RULES[rule]}")
        self.record, self.offset, self.rule = record, offset, rule


_LINE = re.compile(rb"[^\r\n]*(?:\r\n|\r|\n)|[^\r\n]+$")


def lines(data: bytes) -> List[Tuple[int, int, int]]:
    """(start, end of text, end of terminator) of every line; terminators \\n, \\r\\n and a lone \\r."""
    out = []
    for m in _LINE.finditer(data):
        s, t = m.start(), m.end()
        e = t - (2 if data.endswith(b"\r\n", s, t) else 1 if t > s and data[t - 1] in (10, 13) else 0)
        out.append((s, e, t))
    return out


def fastq_to_fasta(data: bytes) -> bytes:
    """The FASTA text of a FASTQ stream; raises FastqError (1-based record, offset of its line 1, rule) if malformed."""
    data = bytes(data)
    ls = lines(data)
    out = []
    for r in range(0, len(ls), 4):
        rec, group = r // 4 + 1, ls[r:r + 4]
        s1, e1, t1 = group[0]
        if s1 == e1:                                        # an empty line 1: only line terminators may follow
            if any(s != e for s, e, _ in ls[r:]):
                raise FastqError(rec, s1, 1)
            break
        if data[s1] != ord("@"):
            raise FastqError(rec, s1, 1)
        if len(group) > 1:
            s2, e2, t2 = group[1]
            if data[s2:e2].lstrip(WS).startswith(b">"):
                raise FastqError(rec, s1, 2)
        if len(group) > 2:
            s3, e3, _ = group[2]
            if not data[s3:e3].startswith(b"+"):
                raise FastqError(rec, s1, 3)
        if len(group) > 3:
            s4, e4, _ = group[3]
            if e4 - s4 != e2 - s2:
                raise FastqError(rec, s1, 4)
        if len(group) < 4:
            raise FastqError(rec, s1, 5)
        out.append(b">" + data[s1 + 1:t2])
    return b"".join(out)


def stats(data: bytes) -> dict:
    """What pk_indexer_fastq_stats reports for a well-formed stream."""
    ls = lines(bytes(data))
    records = 0
    for r in range(0, len(ls), 4):
        if ls[r][0] == ls[r][1]:
            break
        records += 1
    return {"records": records, "lines": len(ls), "bytes_fed": len(data), "bytes_emitted": len(fastq_to_fasta(data))}


def read_set(n_reads: int, length: int = 150, seed: int = 0, genome_bp: int = 1 << 20, sub_rate: float = 0.01,
             n_rate: float = 0.002, crlf: bool = False, genome: np.ndarray = None):
    """(fastq, fasta): n_reads reads of `length` bp sampled from a random genome (or `genome`, base codes 0..3) on either
    strand, with substitution errors and some N; the FASTA is what fastq_to_fasta makes of the FASTQ, built directly
    (fast for large sets)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    if genome is None:
        genome = rng.integers(0, 4, genome_bp, dtype=np.uint8)
    genome_bp = genome.size
    starts = rng.integers(0, genome_bp - length, n_reads)
    codes = genome[starts[:, None] + np.arange(length)]
    rev = rng.random(n_reads) < 0.5
    codes[rev] = 3 - codes[rev, ::-1]
    sub = rng.random(codes.shape) < sub_rate
    codes[sub] = (codes[sub] + rng.integers(1, 4, int(sub.sum()), dtype=np.uint8)) & 3
    seq = acgt[codes]
    seq[rng.random(codes.shape) < n_rate] = ord("N")
    qual = (rng.integers(33, 74, codes.shape, dtype=np.uint8))
    nl = b"\r\n" if crlf else b"\n"
    fq, fa = [], []
    for i in range(n_reads):
        name = b"read%d/%d len=%d" % (i, seed, length)
        s = seq[i].tobytes()
        fq.append(b"@" + name + nl + s + nl + b"+" + nl + qual[i].tobytes() + nl)
        fa.append(b">" + name + nl + s + nl)
    return b"".join(fq), b"".join(fa)


SCAN_RUNS = 1024                                 # k_fq_scan: one thread per run of ceil(n_chunks / 1024) consecutive chunks


def seam_read_set(n_chunks: int, crlf: bool, seed: int, chunk: int = 16384):
    """(fastq, fasta, names_at, placed): reads of 30 .. 250 bp whose FASTQ text has exactly `n_chunks` 16 KiB chunks, for the
    seams between the scan's runs of per = ceil(n_chunks / SCAN_RUNS) chunks (byte offsets B = t * per * chunk).  The
    varied line lengths put the seams into lines of every role; five seams are hand-placed (`placed`: kind -> B):

      "crlf"         a sequence line's CR at B - 1, its LF at B (this record has CR LF lines whatever `crlf` says);
      "at_quality"   a quality line that begins with '@' begins at B;
      "plus_line"    line 3 (the '+') begins at B;
      "empty_read"   a read without bases: line 1 ends with the byte before B, the empty line 2 begins at B;
      "name_across"  line 1 begins five bytes before B.

    `fasta` is what fastq_to_fasta makes of the FASTQ, built directly; names_at[i] is where name i lies in the FASTQ."""
    rng = np.random.default_rng(seed)
    per = -(-n_chunks // SCAN_RUNS)
    run, n_runs = per * chunk, -(-n_chunks // per)
    nl = b"\r\n" if crlf else b"\n"
    pool = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 1 << 20)]
    pool[rng.random(pool.size) < 0.002] = ord("N")
    pool, qpool = pool.tobytes(), rng.integers(33, 74, 1 << 20, dtype=np.uint8).tobytes()
    fq, fa, names_at, placed = [], [], [], {}
    pos, n = 0, 0

    def emit(name, seq, qual, eol=nl):
        nonlocal pos, n
        rec = b"@" + name + eol + seq + eol + b"+" + eol + qual + eol
        names_at.append(pos + 1)
        fq.append(rec)
        fa.append(b">" + name + eol + seq + eol)
        pos += len(rec)
        n += 1

    def random_read():
        length, at, qat = int(rng.integers(30, 251)), int(rng.integers(0, (1 << 20) - 250)), int(rng.integers(0, (1 << 20) - 250))
        emit(b"r%d len=%d" % (n, length), pool[at:at + length], qpool[qat:qat + length])

    def advance_to(start):                       # random reads, then one whose name is padded so that it ends at `start`
        while start - pos > 700:
            random_read()
        pad = start - pos - 2 - 2 * 40 - 4 * len(nl)
        assert pad >= 8, (start, pos)
        emit((b"pad%d_" % n).ljust(pad, b"p"), pool[:40], qpool[:40])
        assert pos == start

    seq, qual = pool[1000:1050], qpool[1000:1050]
    for t, kind in sorted({1: "crlf", n_runs // 3: "at_quality", n_runs // 2: "plus_line", 2 * n_runs // 3: "empty_read", n_runs - 1: "name_across"}.items()):
        B = t * run
        placed[kind] = B
        if kind == "crlf":
            advance_to(B - 4 - len(b"placed_crlf") - len(seq))
            emit(b"placed_crlf", seq, qual, b"\r\n")
        elif kind == "at_quality":
            advance_to(B - (2 + len(b"placed_at") + len(seq) + 3 * len(nl)))
            emit(b"placed_at", seq, b"@" + qual[1:])
        elif kind == "plus_line":
            advance_to(B - (1 + len(b"placed_plus") + len(seq) + 2 * len(nl)))
            emit(b"placed_plus", seq, qual)
        elif kind == "empty_read":
            advance_to(B - (1 + len(b"placed_empty") + len(nl)))
            emit(b"placed_empty", b"", b"")
        else:
            advance_to(B - 5)
            emit(b"placed_name_across the seam", seq, qual)
    assert len(placed) == 5
    while pos <= (n_chunks - 1) * chunk:
        random_read()
    fq, fa = b"".join(fq), b"".join(fa)
    assert -(-len(fq) // chunk) == n_chunks
    return fq, fa, np.array(names_at, dtype=np.uint64), placed


# ------------------------------------------------------------------ hand-written cases
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

# .kin.json fields that depend on the counts alone (not on the input file, the clock or the host)
DETERMINISTIC = ("chromosomes", "data_size", "file_ver", "flush_every", "frag_size", "hist", "hist_count", "hist_max", "hist_min",
                 "hist_sum", "kmer_len", "kmer_size", "max_size", "num_kmers", "output_file_cheksum", "output_file_size",
                 "vals_count", "vals_max", "vals_min", "vals_sum")
