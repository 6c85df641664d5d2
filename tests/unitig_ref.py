"""The unitig definition of the README ("Unitigs") in plain Python, over a dict of canonical addresses: the yardstick of
unitigs.py and pk_unitig.  It works on integers from out() and in_() as the definition states them and knows nothing of the
kernels' link bytes.

    expected(counts, k, min_count, max_count, min_kmers) -> dict(first_addr, n_kmers, depth (U,) uint64, circular (U,) uint8,
        fasta (bytes), n_nodes, n_branching, n_linear, n_circular, n_short, nodes_short, longest_kmers, paths)
`counts`: {canonical address: table byte} (bytes outside the window, and addresses that are not canonical, are no nodes);
`paths`: per written row the oriented k-mers o_1 .. o_n.
"""
import numpy as np

LETTERS = "ACGT"


_RC4 = []
for _v in range(256):                                        # the reverse complement of 4 bases
    _RC4.append(sum((3 - ((_v >> (2 * _i)) & 3)) << (2 * (3 - _i)) for _i in range(4)))


def rc(o: int, k: int) -> int:
    r, chunks = 0, (k + 3) // 4                              # o padded with A in front to whole bytes: the pad comes out as T behind
    for _ in range(chunks):
        r = (r << 8) | _RC4[o & 255]
        o >>= 8
    return r >> (2 * (4 * chunks - k))


def canon(o: int, k: int) -> int:
    return min(o, rc(o, k))


def encode(text: str) -> int:
    o = 0
    for ch in text:
        o = (o << 2) | LETTERS.index(ch)
    return o


def decode(o: int, k: int) -> str:
    return "".join(LETTERS[(o >> (2 * (k - 1 - i))) & 3] for i in range(k))


def kmers_of(text: str, k: int):
    """The canonical addresses of the k-mers of a sequence, in order."""
    o, mask, out = 0, 4 ** k - 1, []
    for i, ch in enumerate(text):
        o = ((o << 2) | LETTERS.index(ch)) & mask
        if i >= k - 1:
            out.append(canon(o, k))
    return out


def counts_of_table(table) -> dict:
    table = np.asarray(table)
    return {int(x): int(table[x]) for x in np.flatnonzero(table)}


def table_of(counts: dict, k: int) -> np.ndarray:
    table = np.zeros(4 ** k, dtype=np.uint8)
    for x, v in counts.items():
        table[x] = v
    return table


class Graph:
    def __init__(self, counts: dict, k: int, min_count: int = 1, max_count: int = 255):
        assert k % 2 == 1
        self.k, self.mask = k, 4 ** k - 1
        self.S = {x for x, v in counts.items() if min_count <= v <= max_count and x == canon(x, k)}
        self.oriented = self.S | {rc(x, k) for x in self.S}  # canon(t) in S  <=>  t in oriented

    def out(self, o: int):
        return [t for t in ((((o << 2) | b) & self.mask) for b in range(4)) if t in self.oriented]

    def in_(self, t: int):
        return [rc(u, self.k) for u in self.out(rc(t, self.k))]

    def compactable(self, o: int, t: int) -> bool:
        return self.out(o) == [t] and len(self.in_(t)) == 1 and canon(o, self.k) != canon(t, self.k)

    def succ(self, o: int):
        """t if a compactable edge o -> t leaves o, else None."""
        outs = self.out(o)
        return outs[0] if len(outs) == 1 and self.compactable(o, outs[0]) else None

    def pred(self, t: int):
        """o if a compactable edge o -> t enters t, else None (by the symmetry: rc(t) -> rc(o))."""
        u = self.succ(rc(t, self.k))
        return None if u is None else rc(u, self.k)

    def branching(self, x: int) -> bool:
        return len(self.out(x)) >= 2 or len(self.out(rc(x, self.k))) >= 2


def spell(path, k: int) -> str:
    return decode(path[0], k) + "".join(LETTERS[o & 3] for o in path[1:])


def all_unitigs(g: Graph):
    """Every unitig of the graph as (first_addr, circular, path), in row order, before min_kmers."""
    k, used, linear, circular = g.k, set(), [], []
    for x in sorted(g.S):
        if x in used:
            continue
        o, is_cycle = x, False
        while True:                                          # back to where the unitig begins, or once around
            p = g.pred(o)
            if p is None:
                break
            if canon(p, k) == x:
                is_cycle = True
                break
            o = p
        if is_cycle:
            path = [x]
            while True:
                t = g.succ(path[-1])
                assert t is not None
                if t == x:
                    break
                assert canon(t, k) != x, "a cycle meets a node once"
                path.append(t)
            nodes = [canon(q, k) for q in path]
            at = nodes.index(min(nodes))
            assert at == 0, "the nodes are visited in ascending order: the first of a cycle is its minimum"
            circular.append((nodes[0], 1, path))
        else:
            path = [o]
            while True:
                t = g.succ(path[-1])
                if t is None:
                    break
                path.append(t)
            if len(path) == 1:
                path = [canon(path[0], k)]
            elif canon(path[-1], k) < canon(path[0], k):
                path = [rc(q, k) for q in reversed(path)]
            linear.append((canon(path[0], k), 0, path))
        for q in path:
            assert canon(q, k) not in used, "a node lies in one unitig"
            used.add(canon(q, k))
    assert used == g.S
    return sorted(linear) + sorted(circular)


def expected(counts: dict, k: int, min_count: int = 1, max_count: int = 255, min_kmers: int = 1) -> dict:
    g = Graph(counts, k, min_count, max_count)
    rows, n_short, nodes_short, fasta = [], 0, 0, []
    for first, circ, path in all_unitigs(g):
        if len(path) < min_kmers:
            n_short += 1
            nodes_short += len(path)
            continue
        fasta.append(f">{len(rows)}\n{spell(path, k)}\n")
        rows.append((first, len(path), sum(counts[canon(q, k)] for q in path), circ, path))
    return {"first_addr": np.array([r[0] for r in rows], dtype=np.uint64), "n_kmers": np.array([r[1] for r in rows], dtype=np.uint64),
            "depth": np.array([r[2] for r in rows], dtype=np.uint64), "circular": np.array([r[3] for r in rows], dtype=np.uint8),
            "fasta": "".join(fasta).encode("ascii"), "n_nodes": len(g.S), "n_branching": sum(g.branching(x) for x in g.S),
            "n_linear": sum(1 for r in rows if not r[3]), "n_circular": sum(1 for r in rows if r[3]), "n_short": n_short,
            "nodes_short": nodes_short, "longest_kmers": max([r[1] for r in rows], default=0), "paths": [r[4] for r in rows], "graph": g}


def texts(result) -> list:
    """The sequences of a FASTA text of unitigs, the row indices checked."""
    lines = result["fasta"].decode("ascii").split("\n")
    assert lines[-1] == "" and len(lines) % 2 == 1
    for r in range(len(lines) // 2):
        assert lines[2 * r] == f">{r}", (r, lines[2 * r])
    return lines[1:-1:2]


def check_invariants(result, min_kmers: int = 1) -> None:
    """What the definition promises of a result of expected() (min_kmers = 1: every node is in a row)."""
    g, k = result["graph"], result["graph"].k
    seen = []
    for path, first, n, circ, text in zip(result["paths"], result["first_addr"], result["n_kmers"], result["circular"], texts(result)):
        nodes = [canon(o, k) for o in path]
        seen += nodes
        assert len(path) == int(n) >= min_kmers and len(text) == len(path) + k - 1 and kmers_of(text, k) == nodes
        assert all(g.compactable(a, b) for a, b in zip(path, path[1:])), "every consecutive pair is compactable"
        if circ:
            assert g.succ(path[-1]) == path[0] and int(first) == min(nodes) == nodes[0] == path[0]
        else:
            assert g.succ(path[-1]) is None and g.pred(path[0]) is None, "no end is extendable"
            assert int(first) == nodes[0] and (len(path) == 1 and path[0] == nodes[0] or nodes[0] < nodes[-1])
        assert text != decode(rc(encode(text), len(text)), len(text)), "no text equals its own reverse complement"
    assert len(seen) == len(set(seen)), "a node in two rows"
    if min_kmers == 1:
        assert set(seen) == g.S, "every node is in exactly one row"
    assert len(seen) + result["nodes_short"] == result["n_nodes"]
    key = [(int(c), int(a)) for c, a in zip(result["circular"], result["first_addr"])]
    assert key == sorted(key) and len(set(key)) == len(key), "rows: linear by first_addr, then circular by first_addr"
