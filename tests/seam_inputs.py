"""Enumerated FASTQ streams for the seams of the record walkers' 64-position steps (test_seam_inputs_host.py,
test_gpu_walker_seams.py, test_gpu_correct.py).  Nothing here is drawn by chance but the bases themselves.

correct_cases(k, seam, genome, breaker, seed) holds one read per (c, a, b): the one candidate of the read at position c, the
nearest invalid position below it at c - a and above it at c + b.  c takes every value of seam - k - 1 .. seam + k and a
and b every value of 1 .. k and FAR (none within k), so the reads hold every (lane, nl, nr) that kmer_correct.hip's
corr_step can meet at that seam, the runs shorter than k (no candidate) included.  A read is seam + 64 positions cut from
`genome` with one substitution at c; the cover bits are from anywhere: all set but the candidate's.  BREAKERS names what
stands at c - a and c + b: an N, a byte that is neither letter nor blank (0x00 below c and 0xC3 above it, swapped in every
second read), an interior blank, or a base whose quality lies below the threshold T (line 4 holds T - 1 there and T or
more everywhere else).  at_end: the read ends at c + b, so its own end is what ends the run above c -- in the walk's last
step or in the step that flushes it; with b = FAR it ends at c + k + 1.  The lengths c + b hold `seam` itself: a multiple
of 64, and at seam 256 of the round, where the flush step has nothing to load.  Every fourth read has one to three blanks
in front of position 0.  random_half: every second read is random bases, not the genome's, so that unfixable candidates
occur.

trim_cases(seam, seed) holds every one of the 2^10 cover patterns over the positions seam - 5 .. seam + 4 of a read of
valid bases whose other cover bits are zero: alone, with a run of each of TIE_RUNS positions at the read's start (ties,
and near-ties one shorter and one longer, with the runs at the seam; at seam 256, where the reads are long, only the
lengths that are one of these for the pattern at hand), and with TAIL_RUN set positions from seam + 64 on (for the 16
patterns that hold nothing behind the seam, a step without a set bit lies between that run and the pattern).
trim_breakers(seam, seed) puts an N, a blank or a 0x00 on each of the ten positions in turn, where a position that is not
covered is not a zero bit.
"""
import functools

import numpy as np

import correct_inputs
import correct_ref
import trim_ref
from correct_inputs import BLANKS, LETTERS, _substitute

FAR = 0                                                      # "none within k" as a value of a and b
SEAMS = (64, 128, 256)                                       # steps 0 / 1; a step inside a round; TRIM_ROUND, where a round's loads begin
BREAKERS = ("N", "other", "blank", "qual")
T = 53                                                       # the threshold byte of the "qual" cases
TRIM_SEAMS = (64, 256)
WINDOW = 10                                                  # positions seam - 5 .. seam + 4
TIE_RUNS = tuple(range(1, WINDOW + 2))                       # 1 .. 11: one longer than the longest run of a pattern
TAIL_RUN = 3


def triples(k: int, seam: int):
    """Every (c, a, b) of a seam, in the order of the reads."""
    steps = list(range(1, k + 1)) + [FAR]
    return [(c, a, b) for c in range(seam - k - 1, seam + k + 1) for a in steps for b in steps]


def is_candidate(k: int, a: int, b: int) -> bool:
    """The valid run around c, as far as it matters, is min(a, k) - 1 + 1 + min(b, k) - 1 positions long."""
    return (a or k) + (b or k) - 1 >= k


def windows(k: int, a: int, b: int) -> int:
    return (a or k) + (b or k) - k


def correct_cases(k: int, seam: int, genome: bytes, breaker: str, seed: int, at_end: bool = False, random_half: bool = False):
    """(the FASTQ stream, cover (n_bases,) bool, [(c, a, b)] per read)."""
    assert breaker in BREAKERS and seam - k - 1 - k >= 0 and 2 * k < 64
    rng = np.random.default_rng(seed)
    source = np.frombuffer(genome, dtype=np.uint8)
    assert source.size >= seam + 64 and bool(np.isin(source, LETTERS).all())
    recs, cover, cases = [], [], triples(k, seam)
    for i, (c, a, b) in enumerate(cases):
        n = seam + 64 if not at_end else c + (b or k + 1)
        if random_half and i % 2:
            seq = LETTERS[rng.integers(0, 4, n)].copy()
        else:
            at = int(rng.integers(0, source.size - n + 1))
            seq = source[at:at + n].copy()
        _substitute(seq, c, rng)
        qual = rng.integers(T, 127, size=n).astype(np.uint8)
        valid = np.ones(n, dtype=bool)
        broken = [p for p in ((c - a) if a else -1, (c + b) if b else -1) if 0 <= p < n]
        assert len(broken) == (a != FAR) + (b != FAR and not at_end)
        for p in broken:
            valid[p] = False
            if breaker == "N":
                seq[p] = ord("N")
            elif breaker == "other":
                seq[p] = (0x00, 0xC3)[(int(p > c) + i) % 2]
            elif breaker == "blank":
                seq[p] = BLANKS[int(rng.integers(0, len(BLANKS)))]
            else:
                qual[p] = T - 1
        lead = bytes(BLANKS[int(j)] for j in rng.integers(0, len(BLANKS), size=1 + i % 3)) if i % 4 == 3 else b""
        bits = valid.copy()
        bits[c] = False
        cover.append(bits[valid])
        name = b"@c%d a%d b%d" % (c, a, b)
        recs.append(name + b"\n" + lead + seq.tobytes() + b"\n+\n" + bytes([T + 1]) * len(lead) + qual.tobytes() + b"\n")
    return b"".join(recs), np.concatenate(cover), cases


def threshold_of(breaker: str) -> int:
    return T if breaker == "qual" else 0


def _read(rng, n: int, i: int) -> bytes:
    seq = LETTERS[rng.integers(0, 4, n)].tobytes()
    return b"@t%d\n" % i + seq + b"\n+\n" + b"I" * n + b"\n"


def near_ties(pattern: int):
    """The runs at the start that tie with a run of the pattern, or are one shorter or one longer."""
    return tuple(sorted({h for _, n in pattern_runs(pattern) for h in (n - 1, n, n + 1) if h >= 1}))


def trim_cases(seam: int, seed: int, tie_runs=TIE_RUNS):
    """(the FASTQ stream, cover (n_bases,) bool, [(pattern, run at the start, run at seam + 64)] per read): bit j of the
    pattern is the cover bit of position seam - 5 + j.  tie_runs None: per pattern its near_ties only."""
    rng = np.random.default_rng(seed)
    recs, cover, cases = [], [], []
    lo = seam - WINDOW // 2
    assert WINDOW + 1 < lo - 1                               # a zero bit between the run at the start and the window
    for pattern in range(1 << WINDOW):
        for head, tail in [(0, 0)] + [(h, 0) for h in (near_ties(pattern) if tie_runs is None else tie_runs)] + [(0, TAIL_RUN)]:
            n = seam + 64 + 2 * tail if tail else seam + WINDOW // 2 + 3
            bits = np.zeros(n, dtype=bool)
            bits[:head] = True
            bits[lo:lo + WINDOW] = [(pattern >> j) & 1 for j in range(WINDOW)]
            bits[seam + 64:seam + 64 + tail] = True
            recs.append(_read(rng, n, len(recs)))
            cover.append(bits)
            cases.append((pattern, head, tail))
    return b"".join(recs), np.concatenate(cover), cases


TRIM_BREAKS = (ord("N"), ord(" "), 0x00)


def trim_breakers(seam: int, seed: int):
    """(the FASTQ stream, cover (n_bases,) bool, [(position, byte)] per read): reads of 2 * seam positions (the longer side of
    the seam is kept) with one position of seam - 5 .. seam + 4 that holds no valid base; the cover bits of the others are
    all set, all set but two next to the seam, or drawn at p = 0.7 on the window and set elsewhere."""
    rng = np.random.default_rng(seed)
    recs, cover, cases = [], [], []
    n = 2 * seam
    lo = seam - WINDOW // 2
    for p in range(lo, lo + WINDOW):
        for byte in TRIM_BREAKS:
            for style in range(4):
                rec = bytearray(_read(rng, n, len(recs)))
                at = rec.index(b"\n") + 1
                rec[at + p] = byte
                bits = np.ones(n, dtype=bool)
                if style == 1:
                    bits[[seam - 2, seam + 1]] = False
                elif style >= 2:
                    bits[lo:lo + WINDOW] = rng.random(WINDOW) < 0.7
                recs.append(bytes(rec))
                cover.append(np.delete(bits, p))
                cases.append((p, byte))
    return b"".join(recs), np.concatenate(cover), cases


def pattern_runs(pattern: int):
    """[(first bit, length)] of the runs of set bits of a pattern, lowest first."""
    runs, j = [], 0
    while j < WINDOW:
        if (pattern >> j) & 1:
            s = j
            while j < WINDOW and (pattern >> j) & 1:
                j += 1
            runs.append((s, j - s))
        else:
            j += 1
    return runs


# ------------------------------------------------------------------ the cases that the host and the GPU tests share
KS = (5, 13)
CASES = tuple((seam, breaker, at_end) for seam in SEAMS for breaker in BREAKERS for at_end in (False, True))


@functools.lru_cache(maxsize=None)
def case_tables(k: int):
    """(one dense table, its genome): half full at k = 5 (1 KiB), 0.2 % full at k = 13 (64 MiB), where a wrong base is
    nearly always put back."""
    return correct_inputs.tables(k, 1, seed=800 + k) if k == 5 else correct_inputs.tables(k, 1, seed=800 + k, density=0.002)


def min_windows_of(k: int) -> tuple:
    """The values of M every case runs at: 1, the default (None) and k."""
    return (1, None, k)


@functools.lru_cache(maxsize=None)
def correct_case(k: int, seam: int, breaker: str, at_end: bool):
    i = CASES.index((seam, breaker, at_end))
    return correct_cases(k, seam, case_tables(k)[1], breaker, seed=3000 + 100 * k + i, at_end=at_end, random_half=(k == 5))


@functools.lru_cache(maxsize=None)
def correct_want(k: int, seam: int, breaker: str, at_end: bool, M):
    """The reference of a case: computed once, shared by the tests, never changed."""
    fq, cover, _ = correct_case(k, seam, breaker, at_end)
    return correct_ref.expected(fq, k, case_tables(k)[0], M=M, T=threshold_of(breaker), cover=cover)


@functools.lru_cache(maxsize=None)
def trim_case(seam: int):
    """trim_cases of a seam: every tie length at seam 64; at seam 256, where a read is four times as long, each pattern's
    near ties."""
    return trim_cases(seam, seed=3900 + seam, tie_runs=TIE_RUNS if seam == 64 else None)


@functools.lru_cache(maxsize=None)
def trim_want(seam: int):
    fq, cover, _ = trim_case(seam)
    return trim_ref.runs(fq, cover)


# ------------------------------------------------------------------ sixteen tables
N_SIXTEEN = 16                                               # QUERY_MAX_TABLES: the tables of one correction


@functools.lru_cache(maxsize=None)
def sixteen_tables(k: int = 5, seed: int = 3950):
    """(16 tables, the genome): the k-mers of one genome that fills about half of the canonical addresses, dealt to the tables
    one address each at random, so that the windows of a candidate match in different tables."""
    (full,), genome = correct_inputs.tables(k, 1, seed=seed)
    rng = np.random.default_rng(seed + 1)
    held = np.flatnonzero(full)
    owner = rng.integers(0, N_SIXTEEN, held.size)
    tabs = [np.zeros_like(full) for _ in range(N_SIXTEEN)]
    for t in range(N_SIXTEEN):
        tabs[t][held[owner == t]] = full[held[owner == t]]
    return tabs, genome


@functools.lru_cache(maxsize=None)
def sixteen_stream(k: int = 5, seed: int = 3960) -> bytes:
    """300 reads of 80 bases cut from the genome of sixteen_tables with substitutions at 3 % of the bases."""
    genome = np.frombuffer(sixteen_tables(k)[1], dtype=np.uint8)
    rng = np.random.default_rng(seed)
    at = rng.integers(0, genome.size - 80 + 1, 300)
    clean = b"".join(b"@r%d\n" % i + genome[a:a + 80].tobytes() + b"\n+\n" + b"I" * 80 + b"\n" for i, a in enumerate(at.tolist()))
    return correct_inputs.plant(clean, 0.03, seed + 1)[0]
