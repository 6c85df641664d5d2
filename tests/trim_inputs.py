"""Seeded FASTQ streams and cover bits for the trim tests (test_trim_host.py, test_gpu_trim.py).

stream(k, seed) holds reads whose line 2 has the lengths at which kmer_trim.hip's 64-byte steps change -- 0, 1, k - 1, k, 63,
64, 65, 127, 128, 129 and 1000 -- with each of the three line terminators, blanks in front of, inside and behind the
sequence, Ns, lower case, and bytes >= 0x80 in names, '+' lines and qualities; the last record ends with or without a
terminator.  bits(n_valid_bases, seed) draws the cover bits of such a stream read by read: all set, none set, or each set
with probability 0.9, which makes short runs and frequent ties."""
import numpy as np

BLANKS = b" \t\x0b\x0c\x1c\x1d\x1e\x1f"
EOLS = (b"\n", b"\r\n", b"\r")


def lengths(k: int):
    return (0, 1, k - 1, k, 63, 64, 65, 127, 128, 129, 1000)


def stream(k: int, seed: int, reps: int = 6, final_newline: bool = True) -> bytes:
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGTacgt", dtype=np.uint8)
    recs = []
    order = [n for _ in range(reps) for n in lengths(k)]
    for i, j in enumerate(rng.permutation(len(order))):
        n = order[int(j)]
        eol = EOLS[i % 3]
        seq = letters[rng.choice(8, size=n, p=[0.22, 0.22, 0.22, 0.22, 0.03, 0.03, 0.03, 0.03])].copy()
        if n and i % 3 == 0:                                 # one or two Ns
            seq[rng.integers(0, n, size=int(rng.integers(1, 3)))] = ord("N")
        style = i % 4                                        # 0 plain, 1 blanks in front, 2 behind, 3 in front, inside and behind
        if style == 3 and n >= 3:
            seq[int(rng.integers(1, n - 1))] = BLANKS[int(rng.integers(0, len(BLANKS)))]
        blank = lambda m: bytes(BLANKS[int(b)] for b in rng.integers(0, len(BLANKS), size=m))   # noqa: E731
        line2 = (blank(int(rng.integers(1, 4))) if style in (1, 3) else b"") + seq.tobytes() + (blank(int(rng.integers(1, 4))) if style in (2, 3) else b"")
        qual = rng.integers(33, 127, size=len(line2)).astype(np.uint8)
        high = rng.random(len(line2)) < 0.1
        qual[high] = rng.integers(0x80, 0x100, size=int(high.sum()))
        if len(line2) and i % 7 == 0:
            qual[0] = ord("@")
        name = b"r%d len=%d " % (i, n) + bytes([0x80 + i % 128, 0xC3, 0xA9])
        plus = b"+" + (name if i % 5 == 0 else b"")
        recs.append(b"@" + name + eol + line2 + eol + plus + eol + qual.tobytes() + eol)
    data = b"".join(recs)
    if not final_newline:
        data = data[:-len(EOLS[(len(order) - 1) % 3])]
    return data


def bits(n_valid_bases, seed: int) -> np.ndarray:
    """(sum of n_valid_bases,) bool: per read all set (40 %), none set (15 %), or each set with probability 0.9."""
    rng = np.random.default_rng(seed)
    out = []
    for n in np.asarray(n_valid_bases).tolist():
        u = rng.random()
        out.append(np.ones(n, dtype=bool) if u < 0.40 else np.zeros(n, dtype=bool) if u < 0.55 else rng.random(n) < 0.9)
    return np.concatenate(out) if out else np.zeros(0, dtype=bool)
