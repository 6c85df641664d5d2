"""Inputs of the unitig tests: sequences whose (k-1)-mers are all distinct, also against their reverse complements and
against everything drawn before, so that the graph of their k-mers is exactly the paths and cycles that were drawn (no
spurious edge), and the edge features a test names, found in a reference result."""
import random

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
