"""Inputs of the unitig tests: sequences whose (k-1)-mers are all distinct, also against their reverse complements and
against everything drawn before, so that the graph of their k-mers is exactly the paths and cycles that were drawn (no
spurious edge), and the edge features a test names, found in a reference result."""
import functools
import random

import numpy as np

import unitig_ref as ref


def _canon_at(seq, i, w):
    """The canonical (k-1)-mer at seq[i:i + w]; None for one that is its own reverse complement (k - 1 is even), which would
    make the k-mer in front of it a hairpin."""
    o = ref.encode("".join(seq[i:i + w]))
    r = ref.rc(o, w)
    return None if o == r else min(o, r)


def distinct_sequence(rng: random.Random, length: int, k: int, seen: set, circular: bool = False) -> str:
    """`length` random bases whose canonical (k-1)-mers are new to `seen` (they are added).  circular: also the k - 2
    (k-1)-mers across the seam of the sequence read as a ring; the text returned is the ring cut open, its first k - 1
    bases repeated behind it, whose k-mers are the `length` nodes of the ring."""
    w = k - 1
    for _ in range(50):
        seq, mine, ok = [], set(), True
        while len(seq) < length:
            for b in rng.sample("ACGT", 4):
                seq.append(b)
                if len(seq) < w:
                    break
                c = _canon_at(seq, len(seq) - w, w)
                if c is not None and c not in seen and c not in mine:
                    mine.add(c)
                    break
                seq.pop()
            else:                                            # no base fits here: start again
                ok = False
                break
        ring = [seq[i % length] for i in range(length + w)] if ok and circular else []
        if ring:                                             # the ring's (k-1)-mers, all `length` of them, from scratch
            mine = {_canon_at(ring, i, w) for i in range(length)}
            ok = len(mine) == length and None not in mine and not (mine & seen)
        if ok:
            seen |= mine
            return "".join(ring if circular else seq)
    raise AssertionError("no sequence with distinct (k-1)-mers found")


def counts_of(sequences, k: int, value: int = 1) -> dict:
    counts = {}
    for s in sequences:
        for x in ref.kmers_of(s, k):
            counts[x] = value
    return counts


def features(g) -> set:
    """Which of the edge rules the graph exercises: "self_loop" (o -> o), "hairpin" (o -> rc(o)), "double_edge" (two edges
    between two different nodes: o -> t and t -> o, so both sides of canon(o) lead to canon(t)).
    Two successors t and rc(t) of ONE o cannot exist when k is odd: they would share the prefix w = o[1:], so w[i] =
    comp(w[k - 1 - i]) for 1 <= i <= k - 2, and the middle position i = (k - 1) / 2 would hold its own complement.  That is
    asserted here wherever it is looked for."""
    found = set()
    for x in g.S:
        for o in (x, ref.rc(x, g.k)):
            outs = g.out(o)
            assert not any(ref.rc(t, g.k) in outs for t in outs), "t and rc(t) leave the same k-mer: impossible for odd k"
            if o in outs:
                found.add("self_loop")
            if ref.rc(o, g.k) in outs:
                found.add("hairpin")
            if any(o in g.out(t) and ref.canon(t, g.k) != x for t in outs):
                found.add("double_edge")
    return found


# ------------------------------------------------------------------ the inputs of the seam tests ---
# Every expectation below is computed once per process and shared by test_unitigs_host.py (their preconditions) and
# test_gpu_unitig_seams.py (the comparison); nobody writes to a cached result.
def canonical(k: int) -> list:
    return [x for x in range(4 ** k) if x == ref.canon(x, k)]


K1_WINDOWS = ((1, 1), (1, 255))


def k1_tables() -> list:
    """k = 1: the canonical addresses are 0 (A) and 1 (C); the 9 tables with the bytes 0, 1 or 2 at them."""
    return [{x: v for x, v in ((0, a), (1, c)) if v} for a in range(3) for c in range(3)]


K3_DENSITIES = (0.05, 0.1, 0.15, 0.2, 0.3, 0.5, 0.8)
K3_SUBSETS = 1500


@functools.lru_cache(maxsize=None)
def k3_subsets() -> tuple:
    """k = 3: random subsets of the 32 canonical addresses, the density drawn per subset, the counts from 1 to 3."""
    rng, canon = random.Random(3), canonical(3)
    out = []
    for _ in range(K3_SUBSETS):
        d = rng.choice(K3_DENSITIES)
        out.append({x: rng.randint(1, 3) for x in canon if rng.random() < d})
    return tuple(out)


@functools.lru_cache(maxsize=None)
def k3_cases() -> tuple:
    """(name, counts, min, max, expected) in the order one builder runs them: every subset under the window 1-255, every
    third one also under 2-3 right behind it."""
    out = []
    for i, counts in enumerate(k3_subsets()):
        for mn, mx in ((1, 255),) + (((2, 3),) if i % 3 == 0 else ()):
            out.append((f"subset {i} window {mn}-{mx}", counts, mn, mx, ref.expected(counts, 3, mn, mx)))
    return tuple(out)


RING_K, RING_COUNT, LINE_COUNT = 11, 2, 5
N_RINGS, N_LINES = 1100, 95


@functools.lru_cache(maxsize=None)
def ring_table() -> dict:
    """k = 11: 1100 rings of k to 2k nodes (shorter ones run out of distinct (k-1)-mers) with the count 2, and 95 paths of
    1 to 2k nodes with the count 5; nothing branches.  The window 1-2 holds the rings alone, 5-5 the paths alone."""
    k, rng, seen = RING_K, random.Random(11), set()
    rings = [distinct_sequence(rng, rng.randint(k, 2 * k), k, seen, circular=True) for _ in range(N_RINGS)]
    lines = [distinct_sequence(rng, rng.randint(k, 3 * k - 1), k, seen) for _ in range(N_LINES)]
    counts = counts_of(rings, k, RING_COUNT)
    counts.update(counts_of(lines, k, LINE_COUNT))
    return counts


@functools.lru_cache(maxsize=None)
def ring_expected(mn: int = 1, mx: int = 255, M: int = 1) -> dict:
    return ref.expected(ring_table(), RING_K, mn, mx, M)


# (min, max, M) of the builds on ring_table(): the rings alone (no linear unitig at all), everything, both with M = 12,
# and the paths alone (no loop candidate at all)
RING_BUILDS = ((1, 2, 1), (1, 255, 1), (1, 2, 12), (1, 255, 12), (5, 5, 1))
# one builder, in this order: it shrinks and grows.  200-255 holds no node; M = 23 is above every unitig (2k = 22 at most)
REBUILDS = ((1, 255, 1), (1, 2, 1), (5, 5, 1), (200, 255, 1), (1, 255, 1), (1, 255, 23))


def linear_bytes(want) -> int:
    """The bytes of the linear rows' records in the text of a reference result: where the circular part begins."""
    lin = sum(len(f">{r}\n") + int(n) + want["graph"].k for r, n in enumerate(want["n_kmers"][:want["n_linear"]]))
    assert lin == len(want["fasta"]) or want["fasta"][lin:].startswith(f">{want['n_linear']}\n".encode("ascii"))
    return lin


def loop_candidate_groups(want, group: int = 256) -> set:
    """The groups of `group` consecutive loop candidates -- the nodes of all rings, ascending -- that hold a ring's minimum."""
    k = want["graph"].k
    rings = [path for path, c in zip(want["paths"], want["circular"]) if c]
    nodes = sorted(ref.canon(o, k) for path in rings for o in path)
    at = {x: i for i, x in enumerate(nodes)}
    return {at[path[0]] // group for path in rings}


WIDE_RINGS = 3000


@functools.lru_cache(maxsize=None)
def wide_ring_table() -> dict:
    """k = 11: 3000 rings and nothing else.  A ring's smallest address is the minimum of a dozen or two random addresses,
    so the minima crowd the low third of the loop candidates: the 1100 rings of ring_table() reach 21 groups of 256
    candidates, these reach more than 50."""
    k, rng, seen = RING_K, random.Random(12), set()
    return counts_of([distinct_sequence(rng, rng.randint(k, 2 * k), k, seen, circular=True) for _ in range(WIDE_RINGS)], k, RING_COUNT)


@functools.lru_cache(maxsize=None)
def wide_ring_expected(M: int = 1) -> dict:
    return ref.expected(wide_ring_table(), RING_K, 1, 255, M)


D_K, D_DENSITY, D_SEED = 11, 0.14, 1100


@functools.lru_cache(maxsize=None)
def dense_table() -> np.ndarray:
    """k = 11: the canonical addresses in ascending order, each kept with probability 0.14, the count of x is 1 + x % 5."""
    x = np.arange(4 ** D_K, dtype=np.int64)
    r, rest = np.zeros_like(x), x.copy()
    for _ in range(D_K):                                     # the reverse complement, base by base
        r = (r << 2) | (3 - (rest & 3))
        rest >>= 2
    canon = x[x < r]
    assert canon.size == 4 ** D_K // 2 and all(int(c) == ref.canon(int(c), D_K) for c in canon[::4099])
    kept = canon[np.random.default_rng(D_SEED).random(canon.size) < D_DENSITY]
    table = np.zeros(4 ** D_K, dtype=np.uint8)
    table[kept] = 1 + kept % 5
    return table


@functools.lru_cache(maxsize=None)
def dense_expected(M: int = 1) -> dict:
    return ref.expected(ref.counts_of_table(dense_table()), D_K, 1, 255, M)


def ends_of(want) -> set:
    """The ends of the linear unitigs of a reference result built with min_kmers = 1."""
    k = want["graph"].k
    return {ref.canon(path[i], k) for path in want["paths"][:want["n_linear"]] for i in (0, -1)}
