"""Every shape the partition plan of a feed can take (make_part_plan and the two launcher choices, as
pk_diag_plan_slice reports them), one case per shape, and texts that keep the tested address slice busy.

A plan's CLASS is what decides which kernels and which branches of them a feed runs: the k_walk_sort instantiation, the
number of sort levels, where the final buckets' rooms come from, sampled or exact layout, the bucket-count kernel, and
whether the table has fewer than 16 addresses.  CASES holds one (k, n_slices, slice, n_bytes) per class of the lattice
that tests/test_plan_host.py enumerates (every legal k and slice count, feeds up to 20 MiB); that test fails when a class
has no case or a case no longer lies in the class it is listed under."""
import functools

import numpy as np

import synth

LINE = 71                                                    # 70 columns and the line feed
CHUNK = 16384
SAMPLED_FROM = 1023 * CHUNK + 1                              # the smallest feed of 1024 chunks: sampled layout
FEED_CAP = 20 << 20                                          # the lattice ends here (larger plans: the full-size tests)
HOT_COPIES = 320                                             # of one unit: its windows saturate, byte counters wrap


def plan_class(d: dict) -> tuple:
    """(variant, levels, rooms, sampled, count kernel, tiny) of a pk_diag_plan_slice answer."""
    levels = 0 if d["b1"] == 0 else 1 if d["b2"] == 0 else 2
    if levels < 2:
        rooms = "l1"
    elif d["sample2"]:
        rooms = "sample2"
    else:
        rooms = "final" if d["n_tally"] == d["B1"] * d["B2"] else "none"     # "none": part_plan_check refuses it
    return (d["variant"], levels, rooms, d["sample_stride"] == 16, d["count_kernel"], d["addr_bits"] < 4)


def text_floor(k: int) -> int:
    """The smallest text focused_text builds: the hot record, a synth stretch, the poly-A line, headers and some filler."""
    return HOT_COPIES * (k + 4) + 2500


# class -> (k, n_slices, slice, n_bytes).  n_bytes: the smallest feed of the class (or text_floor(k), for the classes that
# begin at one byte), rounded up to whole lines.  Where several (k, n_slices) reach the class with that feed, the largest
# table of at most 2^26 bytes (else the smallest), then the smallest k.  The slice's address prefix reads ACGTACGT...
# (CAGT... for fewer than 16 slices), cut to the slice bits: canonical k-mers seldom begin with G or T.
# Bytes classes: the hot unit's k-mers (HOT_COPIES windows each) lie in one final bucket by construction, so every one of
# these texts holds a 255-fold k-mer in one bucket and buckets_recounted >= 1 is asserted for all of them.
CASES = {
    ("deep", 1, "l1", False, "bytes", False): (19, 8192, 867, 9869),
    ("deep", 1, "l1", False, "whole", False): (19, 65536, 6939, 524335),
    ("deep", 1, "l1", True, "whole", False): (19, 8192, 867, 16760899),
    ("deep", 2, "final", False, "bytes", False): (19, 4096, 433, 9869),
    ("deep", 2, "final", False, "whole", False): (19, 4096, 433, 8388650),
    ("deep", 2, "final", True, "bytes", False): (19, 2048, 216, 16760899),
    ("deep", 2, "final", True, "whole", False): (19, 4096, 433, 16760899),
    ("deep", 2, "sample2", False, "bytes", False): (19, 128, 13, 9869),
    ("deep", 2, "sample2", True, "bytes", False): (19, 128, 13, 16760899),
    ("k15", 2, "final", False, "bytes", False): (15, 1, 0, 8591),
    ("k15", 2, "final", True, "bytes", False): (15, 1, 0, 16760899),
    ("k17", 2, "sample2", False, "bytes", False): (17, 1, 0, 9230),
    ("k17", 2, "sample2", True, "bytes", False): (17, 1, 0, 16760899),
    ("narrow", 0, "l1", False, "whole", False): (7, 1, 0, 6035),
    ("narrow", 0, "l1", False, "whole", True): (1, 1, 0, 4118),
    ("narrow", 0, "l1", True, "whole", False): (7, 1, 0, 16760899),
    ("narrow", 0, "l1", True, "whole", True): (1, 1, 0, 16760899),
    ("narrow", 1, "l1", False, "bytes", False): (11, 1, 0, 7313),
    ("narrow", 1, "l1", False, "whole", False): (9, 1, 0, 32802),
    ("narrow", 1, "l1", True, "whole", False): (11, 1, 0, 16760899),
    ("narrow", 2, "final", False, "bytes", False): (13, 1, 0, 7952),
    ("narrow", 2, "final", False, "half", False): (13, 1, 0, 8388650),
    ("narrow", 2, "final", True, "half", False): (13, 1, 0, 16760899),
    ("narrow_sliced", 0, "l1", False, "bytes", False): (9, 4, 1, 6674),
    ("narrow_sliced", 0, "l1", False, "half", False): (9, 8, 2, 6674),
    ("narrow_sliced", 0, "l1", False, "whole", False): (9, 4, 1, 8236),
    ("narrow_sliced", 0, "l1", False, "whole", True): (3, 8, 2, 4757),
    ("narrow_sliced", 0, "l1", True, "half", False): (9, 8, 2, 16760899),
    ("narrow_sliced", 0, "l1", True, "whole", False): (9, 4, 1, 16760899),
    ("narrow_sliced", 0, "l1", True, "whole", True): (3, 8, 2, 16760899),
    ("narrow_sliced", 1, "l1", False, "bytes", False): (13, 8, 2, 7952),
    ("narrow_sliced", 1, "l1", False, "whole", False): (9, 2, 0, 16401),
    ("narrow_sliced", 1, "l1", True, "whole", False): (13, 8, 2, 16760899),
    ("narrow_sliced", 2, "final", False, "bytes", False): (15, 16, 1, 8591),
    ("narrow_sliced", 2, "final", False, "half", False): (13, 4, 1, 2097198),
    ("narrow_sliced", 2, "final", True, "bytes", False): (15, 8, 2, 16760899),
    ("narrow_sliced", 2, "final", True, "half", False): (15, 16, 1, 16760899),
    ("wide_sliced", 1, "l1", False, "bytes", False): (17, 512, 54, 9230),
    ("wide_sliced", 1, "l1", False, "whole", False): (17, 65536, 6939, 32802),
    ("wide_sliced", 1, "l1", True, "whole", False): (17, 512, 54, 16760899),
    ("wide_sliced", 2, "final", False, "bytes", False): (17, 256, 27, 9230),
    ("wide_sliced", 2, "final", False, "whole", False): (17, 256, 27, 8388650),
    ("wide_sliced", 2, "final", True, "bytes", False): (17, 128, 13, 16760899),
    ("wide_sliced", 2, "final", True, "whole", False): (17, 256, 27, 16760899),
    ("wide_sliced", 2, "sample2", False, "bytes", False): (17, 8, 2, 9230),
    ("wide_sliced", 2, "sample2", True, "bytes", False): (17, 8, 2, 16760899),
}


def case_id(case) -> str:
    k, n_slices, s, n_bytes = case
    return f"k{k}-{n_slices}sl-s{s}-{n_bytes}B"


def slice_bits(n_slices: int) -> int:
    return n_slices.bit_length() - 1


def slice_prefix(k: int, n_slices: int, s: int) -> bytes:
    """The ceil(slice_bits / 2) leading bases of the k-mers of slice `s` (a free low bit of the last one reads 0)."""
    sb = slice_bits(n_slices)
    p = (sb + 1) // 2
    top = s << (2 * p - sb)
    return bytes(b"ACGT"[(top >> (2 * (p - 1 - i))) & 3] for i in range(p))


def preferred_slice(n_slices: int) -> int:
    """The slice whose prefix reads ACGTACGT (CAGTCAGT for fewer than 16 slices), cut to the slice bits."""
    sb = slice_bits(n_slices)
    pattern = 0x1B1B if sb >= 4 else 0x4B4B
    return pattern >> (16 - sb)


def _wrap(seq: np.ndarray) -> np.ndarray:
    """seq on lines of 70 columns, each with its line feed (the last line padded with N)."""
    rows = -(-seq.size // (LINE - 1))
    out = np.full((rows, LINE), ord("N"), dtype=np.uint8)
    out[:, LINE - 1] = ord("\n")
    flat = np.full(rows * (LINE - 1), ord("N"), dtype=np.uint8)
    flat[:seq.size] = seq
    out[:, :LINE - 1] = flat.reshape(rows, LINE - 1)
    return out.reshape(-1)


def _units(rng, prefix: bytes, k: int, m: int) -> np.ndarray:
    """m units of prefix + (k - len(prefix) + 3) random bases + N, back to back."""
    p = len(prefix)
    u = np.empty((m, k + 4), dtype=np.uint8)
    u[:, :p] = np.frombuffer(prefix, dtype=np.uint8)
    u[:, p:k + 3] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(m, k + 3 - p))]
    u[:, k + 3] = ord("N")
    return u.reshape(-1)


@functools.lru_cache(maxsize=4)
def focused_text(k: int, n_slices: int, s: int, n_bytes: int, seed: int) -> bytes:
    """A FASTA text of exactly n_bytes whose windows concentrate in slice `s` of n_slices at kmer_len k.

    Four records and what synth brings: one unit (the slice's address prefix + k - prefix + 3 random bases, fixed by
    (k, n_slices, s) alone, so texts of different seeds share it) HOT_COPIES times with an N between the copies; a stretch of
    synth.generate with tandem repeats, duplications, N gaps and lower case (side list, record structure); a poly-A line
    when the slice is 0; and random units of the same form, N-joined on 70-column lines, up to the length asked for."""
    assert n_bytes >= text_floor(k), (k, n_bytes)
    prefix = slice_prefix(k, n_slices, s)
    hot_rng = np.random.default_rng([k, n_slices, s])
    while True:                                              # a unit whose first window is its own canonical form: it lies in the slice
        hot = _units(hot_rng, prefix, k, 1)
        first = hot[:k].tobytes()
        if first <= first.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]:
            break
    parts = [np.frombuffer(b">hot unit\n", dtype=np.uint8), _wrap(np.tile(hot, HOT_COPIES))]
    body, _ = synth.generate(seed, min(20_000, max(600, n_bytes // 8)), 2, pm_tandem=100, pm_dup=100, pm_ngap=30, pm_lower=50)
    parts.append(np.asarray(body, dtype=np.uint8))
    if body[-1] != ord("\n"):
        parts.append(np.frombuffer(b"\n", dtype=np.uint8))
    if s == 0:
        parts.append(np.frombuffer(b">polyA\n" + b"A" * 400 + b"\n", dtype=np.uint8))
    parts.append(np.frombuffer(b">units\n", dtype=np.uint8))
    left = n_bytes - sum(p.size for p in parts)
    assert left >= 2, (k, n_bytes, left)
    rng = np.random.default_rng([seed, k, n_slices, s])
    fill = _wrap(_units(rng, prefix, k, left // (k + 4) + 1))[:left].copy()
    if fill[-2] == ord("\n"):                                # the cut fell right behind a line feed: no blank line
        fill[-2] = ord("N")
    fill[-1] = ord("\n")
    parts.append(fill)
    text = np.concatenate(parts).tobytes()
    assert len(text) == n_bytes
    return text
