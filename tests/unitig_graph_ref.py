"""The graph definition of the README ("Unitigs", the edges) in plain Python over sets, on a result of unitig_ref.expected():
the yardstick of unitigs.py --gfa and pk_unitig_graph.  It knows nothing of link bytes or candidates.

    graph(want) -> dict(edges [(from, from_sign, to, to_sign, b)], edge_from, edge_to (E,) uint64, edge_orient (E,) uint8,
        n_edges, edges_dropped, n_dead_ends, gfa (bytes), tails {oriented k-mer: (row, sign)})
Signs are 0 for + and 1 for -; b is the base of the successor.  `want` is a result of unitig_ref.expected() with any min_kmers;
the unitigs that min_kmers dropped are found again from its graph.

    parse_gfa(data) -> dict(segments [(name, text, LN, KC)], links [(from, from_sign, to, to_sign, overlap)])
"""
import numpy as np

import unitig_ref as ref

HEADER = b"H\tVN:Z:1.0\n"


def rc_text(text: str) -> str:
    return text[::-1].translate(str.maketrans("ACGT", "TGCA"))


def tails_of(paths, k: int) -> dict:
    """{tail(r,+) = o_1: (r, 0), tail(r,-) = rc(o_n): (r, 1)} over the paths; the 2U tails are different oriented k-mers."""
    tails = {}
    for r, path in enumerate(paths):
        for o, sign in ((path[0], 0), (ref.rc(path[-1], k), 1)):
            assert o not in tails, "two oriented rows share a tail"
            tails[o] = (r, sign)
    return tails


def head(path, sign: int, k: int) -> int:
    return ref.rc(path[0], k) if sign else path[-1]


def graph(want) -> dict:
    g, k, paths = want["graph"], want["graph"].k, want["paths"]
    tails = tails_of(paths, k)
    every = tails_of([path for _, _, path in ref.all_unitigs(g)], k)         # the dropped unitigs too
    edges, dropped, dead = [], 0, 0
    for r, path in enumerate(paths):
        for sign in (0, 1):
            h, before = head(path, sign, k), len(edges)
            for b in range(4):
                t = ((h << 2) | b) & g.mask
                if t not in g.oriented:
                    continue
                assert t in every, "a successor of a unitig end is the tail of exactly one oriented unitig"
                if not want["circular"][r]:
                    assert not g.compactable(h, t), "no edge that leaves a linear head is compactable"
                if t in tails:
                    edges.append((r, sign) + tails[t] + (b,))
                else:
                    dropped += 1
            dead += len(edges) == before
    lines = [HEADER]
    for r, (text, n, depth) in enumerate(zip(ref.texts(want), want["n_kmers"], want["depth"])):
        lines.append(f"S\t{r}\t{text}\tLN:i:{int(n) + k - 1}\tKC:i:{int(depth)}\n".encode("ascii"))
    for r, s, q, u, _ in edges:
        lines.append(f"L\t{r}\t{'+-'[s]}\t{q}\t{'+-'[u]}\t{k - 1}M\n".encode("ascii"))
    return {"edges": edges, "edge_from": np.array([e[0] for e in edges], dtype=np.uint64), "edge_to": np.array([e[2] for e in edges], dtype=np.uint64),
            "edge_orient": np.array([e[1] | (e[3] << 1) for e in edges], dtype=np.uint8), "n_edges": len(edges), "edges_dropped": dropped,
            "n_dead_ends": dead, "gfa": b"".join(lines), "tails": tails}


def parse_gfa(data: bytes) -> dict:
    """The segments and links of a GFA 1.0 text as unitigs.py writes it: the header first, then every S-line, then every L-line."""
    assert data.startswith(HEADER) and data.endswith(b"\n")
    segments, links = [], []
    for line in data[len(HEADER):-1].decode("ascii").split("\n") if len(data) > len(HEADER) else []:
        f = line.split("\t")
        if f[0] == "S":
            assert not links and len(f) == 5 and f[3].startswith("LN:i:") and f[4].startswith("KC:i:"), line
            segments.append((f[1], f[2], int(f[3][5:]), int(f[4][5:])))
        else:
            assert f[0] == "L" and len(f) == 6 and f[2] in "+-" and f[4] in "+-" and f[5].endswith("M"), line
            links.append((int(f[1]), "+-".index(f[2]), int(f[3]), "+-".index(f[4]), int(f[5][:-1])))
    return {"segments": segments, "links": links}


def count_identity(want) -> int:
    """sum over x in S of |out(x)| + |out(rc(x))|, minus 2 * sum over the rows of (n_kmers - 1): n_edges at min_kmers = 1."""
    g = want["graph"]
    return sum(len(g.out(x)) + len(g.out(ref.rc(x, g.k))) for x in g.S) - 2 * int((want["n_kmers"].astype(np.int64) - 1).sum())


def check_overlaps(parsed, g) -> None:
    """Every L-line: the last k - 1 letters of the oriented from-text are the first k - 1 of the oriented to-text, and the k-mer
    across the junction is a node."""
    k = g.k
    texts = [s[1] for s in parsed["segments"]]
    for r, s, q, u, overlap in parsed["links"]:
        a, b = rc_text(texts[r]) if s else texts[r], rc_text(texts[q]) if u else texts[q]
        assert overlap == k - 1 and a[len(a) - (k - 1):] == b[:k - 1], (r, s, q, u)
        assert ref.encode((a + b[k - 1:])[len(a) - k + 1:len(a) + 1]) in g.oriented, (r, s, q, u)


def check_invariants(want, got, min_kmers: int = 1) -> None:
    """What the definition promises of graph(want) = got."""
    g, k = want["graph"], want["graph"].k
    edges = got["edges"]
    assert len(got["tails"]) == 2 * len(want["paths"]), "the tails are unique"
    keys = [(r, s, b) for r, s, _, _, b in edges]
    assert keys == sorted(keys) and len(set(keys)) == len(keys), "the order is total"
    pairs = [e[:4] for e in edges]
    assert len(set(pairs)) == len(pairs), "an edge twice"
    have = set(pairs)
    for r, s, q, u in pairs:
        assert (q, 1 - u, r, 1 - s) in have, "closed under mirroring"
    selfs = [(r, s, q, u) for r, s, q, u in pairs if (q, 1 - u, r, 1 - s) == (r, s, q, u)]
    assert all(r == q and s != u for r, s, q, u in selfs), "an edge that is its own mirror is a hairpin at a unitig end"
    for r, circ in enumerate(want["circular"]):
        if circ:
            assert [e for e in pairs if r in (e[0], e[2])] == [(r, 0, r, 0), (r, 1, r, 1)], "a circular row has its closing edge, both ways"
    counts = {}
    for r, s, _, _ in pairs:
        counts[r] = counts.get(r, 0) + 1
    assert max(counts.values(), default=0) <= 8
    assert got["n_dead_ends"] == 2 * len(want["paths"]) - len({e[:2] for e in pairs})
    if min_kmers == 1:
        assert got["edges_dropped"] == 0 and got["n_edges"] == count_identity(want), "the count identity"
    parsed = parse_gfa(got["gfa"])
    assert [s[1] for s in parsed["segments"]] == ref.texts(want) and [s[0] for s in parsed["segments"]] == [str(r) for r in range(len(want["paths"]))]
    assert [s[2] for s in parsed["segments"]] == [len(s[1]) for s in parsed["segments"]] and [s[3] for s in parsed["segments"]] == want["depth"].tolist()
    assert [e[:4] for e in parsed["links"]] == pairs
    check_overlaps(parsed, g)
