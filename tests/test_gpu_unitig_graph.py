"""pk_unitig_graph and unitigs.py --gfa on the GPU against tests/unitig_graph_ref.py: the three edge arrays, the three totals
and the GFA bytes are compared for equality.  Every test first asserts on the reference alone that its input holds the
feature it is named for."""
import functools
import json
import random

import numpy as np
import pytest

import gpu_support as gs
import synth
import unitig_graph_ref as gref
import unitig_inputs as ui
import unitig_ref as ref
from unitig_support import read_out, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    return gs.lib()


def read_graph(u, got):
    """The graph of the build whose totals are `got`, on the builder u: its totals, its edges, its text and its timings."""
    got.update(u.graph())
    got.update(u.edges())
    got["gfa"] = u.gfa_text().tobytes()
    got["graph_timings"] = u.graph_timings()
    return got


def graph_at(ptr, k, mn=1, mx=255, M=1):
    with gs.lib().Unitigs(k, device=0) as u:
        return read_graph(u, read_out(u, u.build(ptr, mn, mx, M)))


def same_graph(got, want_graph):
    for key in ("n_edges", "edges_dropped", "n_dead_ends"):
        assert got[key] == want_graph[key], (key, got[key], want_graph[key])
    for key in ("edge_from", "edge_to", "edge_orient"):
        assert got[key].dtype == want_graph[key].dtype and got[key].shape == want_graph[key].shape, (key, got[key].dtype, got[key].shape, want_graph[key].shape)
        assert np.array_equal(got[key], want_graph[key]), (key, np.flatnonzero(got[key] != want_graph[key])[:5], got[key][:8], want_graph[key][:8])
    assert got["gfa_bytes"] == len(want_graph["gfa"]), ("gfa_bytes", got["gfa_bytes"], len(want_graph["gfa"]))
    if got["gfa"] != want_graph["gfa"]:
        at = next(i for i, (a, b) in enumerate(zip(got["gfa"], want_graph["gfa"])) if a != b)
        raise AssertionError(("gfa", at, got["gfa"][max(0, at - 60):at + 60], want_graph["gfa"][max(0, at - 60):at + 60]))


def check(counts, k, mn=1, mx=255, M=1, want=None, want_graph=None):
    want = want or ref.expected(counts, k, mn, mx, M)
    want_graph = want_graph or gref.graph(want)
    with gs.Device([ref.table_of(counts, k)]) as dev:
        got = graph_at(dev.ptrs[0], k, mn, mx, M)
    same(got, want)
    same_graph(got, want_graph)
    return got


def out_degrees(want_graph) -> dict:
    deg = {}
    for e in want_graph["edges"]:
        deg[e[0]] = deg.get(e[0], 0) + 1
    return deg


# ------------------------------------------------------------------ 1. every edge rule -------------
def _ring_case(k, seed):
    """A ring of 41 nodes beside a path that holds the table's lowest node."""
    rng, seen = random.Random(seed), set()
    low = "A" * (k - 1) + "C" + "G" * 3
    for i in range(len(low) - k + 2):
        seen.add(ui._canon_at(list(low), i, k - 1))
    return ui.counts_of([low, ui.distinct_sequence(rng, 41, k, seen, circular=True)], k)


@functools.lru_cache(maxsize=None)
def edge_cases(k):
    rng = random.Random(500 + k)
    cases = {"ACACACAC": ui.counts_of(["ACACACAC"], 5), "AAAAATTTTT": ui.counts_of(["AAAAATTTTT"], 5)} if k == 5 else {}
    cases["ring"] = _ring_case(k, 40 + k)
    for d in (0.02, 0.1, 0.3, 0.6, 1.0):
        cases[f"random {d}"] = {x: 1 + x % 7 for x in range(4 ** k) if x == ref.canon(x, k) and (d == 1.0 or rng.random() < d)}
    out = {}
    for name, c in cases.items():
        want = ref.expected(c, k)
        out[name] = (c, want, gref.graph(want))
    return out


def test_edge_cases_hold_every_rule():
    """The precondition of test_every_edge_rule, on the reference alone: a self-loop edge r+ -> r+ of a linear row, a hairpin
    edge r+ -> r- or r- -> r+, a double edge between two nodes, a 2-cycle and a longer ring as circular rows with their two
    edges, and rows with 8 outgoing edges."""
    found = set()
    for k in (5, 7):
        for name, (counts, want, g) in edge_cases(k).items():
            gref.check_invariants(want, g)
            found |= ui.features(want["graph"]) & {"double_edge"}
            for r, s, q, u, _ in g["edges"]:
                if r == q and not want["circular"][r]:
                    found.add("self_loop" if s == u else "hairpin")
                if r == q and want["circular"][r]:
                    found.add("2-cycle" if want["n_kmers"][r] == 2 else "ring")
            if 8 in out_degrees(g).values():
                found.add("8 out")
    assert found == {"self_loop", "hairpin", "double_edge", "2-cycle", "ring", "8 out"}, found


@pytest.mark.parametrize("k", [5, 7])
def test_every_edge_rule(gpu, k):
    for name, (counts, want, g) in edge_cases(k).items():
        check(counts, k, want=want, want_graph=g)


# ------------------------------------------------------------------ 2. --min-kmers -----------------
def test_min_kmers(gpu):
    """M = 1, 2 and 3: an edge into a dropped unitig is counted and not written, the rows of the edges are the new row
    indices; an M above every unitig leaves the header line and no edge."""
    k, rng = 7, random.Random(75)
    counts = {x: 1 for x in range(4 ** 7) if x == ref.canon(x, 7) and rng.random() < 0.1}
    full = ref.expected(counts, k)
    for M in (1, 2, 3, int(full["longest_kmers"]) + 1):
        want = ref.expected(counts, k, 1, 255, M)
        g = gref.graph(want)
        if M == 1:
            assert g["edges_dropped"] == 0 and g["n_edges"] > 100
        elif M <= 3:
            assert g["edges_dropped"] > 0 and g["n_edges"] > 0
            assert not np.array_equal(np.flatnonzero(full["n_kmers"] >= M), np.arange(len(want["n_kmers"])))      # a row index changes
        else:
            assert len(want["n_kmers"]) == 0 and g["gfa"] == gref.HEADER and g["n_edges"] == 0
        got = check(counts, k, M=M, want=want, want_graph=g)
        assert M <= 3 or (got["gfa"] == b"H\tVN:Z:1.0\n" and got["edge_from"].size == 0)


# ------------------------------------------------------------------ 3. window ----------------------
@pytest.mark.parametrize("beside", [2, 3, 250, 251])
def test_window(gpu, beside):
    """A path of 300 nodes of count 250 under the window 3-250 and two k-mers beside it with the count `beside`: inside the
    window they cut the path in three, and the edges at the two cuts join the pieces and the side k-mers; outside it there is
    one row without an edge.  KC of the pieces has five digits."""
    k, mn, mx = 7, 3, 250
    rng, seen = random.Random(77), set()
    path = ui.distinct_sequence(rng, 300 + k - 1, k, seen)
    counts = ui.counts_of([path], k, 250)
    for at, tail in ((100, True), (200, False)):
        kmer = path[at:at + k]
        for b in "ACGT":
            other = kmer[:-1] + b if tail else b + kmer[1:]
            x = ref.canon(ref.encode(other), k)
            if x not in counts:
                counts[x] = beside
                break
    assert len(counts) == 302
    want = ref.expected(counts, k, mn, mx)
    g = gref.graph(want)
    if mn <= beside <= mx:
        assert len(want["n_kmers"]) >= 5 and g["n_edges"] == 8 and g["edges_dropped"] == 0     # a fork and a join: 2 edges each, and their mirrors
        assert sum(10_000 <= int(d) <= 99_999 for d in want["depth"]) >= 2
    else:
        assert want["n_kmers"].tolist() == [300] and g["n_edges"] == 0 and g["n_dead_ends"] == 2 and b"KC:i:75000\n" in g["gfa"]
    check(counts, k, mn, mx, want=want, want_graph=g)


# ------------------------------------------------------------------ 4. digit seams -----------------
SEAM_ROWS = (9, 10, 99, 100, 999, 1000)


def test_digit_seams(gpu):
    """k = 11: the 2048 k-mers over the letters A and C -- every one a row of its own with two successors on either side --
    beside paths of 140 and 10 040 k-mers.  The decimal widths of the row index change inside the S-lines and, as `from` and as
    `to`, inside the L-lines; LN has 2, 3 and 5 digits."""
    k = 11
    rng, seen = random.Random(1111), set()
    crowd = {sum(((v >> (k - 1 - i)) & 1) << (2 * (k - 1 - i)) for i in range(k)) for v in range(2 ** k)}
    assert all(x == ref.canon(x, k) for x in crowd) and len(crowd) == 2048
    for x in crowd:
        text = list(ref.decode(x, k))
        seen.update(c for c in (ui._canon_at(text, 0, k - 1), ui._canon_at(text, 1, k - 1)) if c is not None)
    counts = ui.counts_of([ui.distinct_sequence(rng, 140 + k - 1, k, seen), ui.distinct_sequence(rng, 10_040 + k - 1, k, seen)], k, 3)
    counts.update({x: 1 for x in crowd})
    want = ref.expected(counts, k)
    g = gref.graph(want)
    assert len(want["n_kmers"]) == 2050 and sorted(want["n_kmers"].tolist())[-3:] == [1, 140, 10_040] and g["n_edges"] == 4 * 2048
    for row in SEAM_ROWS:
        assert row in g["edge_from"] and row in g["edge_to"], row
    assert {len(str(int(n) + k - 1)) for n in want["n_kmers"]} == {2, 3, 5}
    check(counts, k, want=want, want_graph=g)


# ------------------------------------------------------------------ 5. lookup at size --------------
@functools.lru_cache(maxsize=None)
def dense_graph():
    return gref.graph(ui.dense_expected(1))


def test_lookup_at_size(gpu):
    """The k = 11 dense table: 278 395 ends to search, more than 1024 workgroups in the scan of the edge counts (two rounds of
    it) and several hundred in those of both kinds of line, and edges whose target is the first end and the last end but one."""
    want, g = ui.dense_expected(1), dense_graph()
    assert (len(want["n_kmers"]), g["n_edges"]) == (227_063, 196_404) and g["edges_dropped"] == 0
    ends = sorted(ui.ends_of(want))
    assert len(ends) > 262_144 and 2 * len(want["n_kmers"]) > 1024 * 256
    at = {x: i for i, x in enumerate(ends)}
    hit = {at[ref.canon(want["paths"][q][-1] if u else want["paths"][q][0], ui.D_K)] for _, _, q, u, _ in g["edges"]}
    # the first candidate is a target; the last one, a dead end of this table, is not, the one before it is: the search ends at
    # either end of the array.  A hit on the very last candidate is test_targets_at_the_ends_of_the_range_k15's: the highest
    # canonical address is the last end there, and a target.
    assert min(hit) == 0 and max(hit) == len(ends) - 2 and len(hit) > 100_000
    with gs.Device([ui.dense_table()]) as dev:
        got = graph_at(dev.ptrs[0], ui.D_K)
    same(got, want)
    same_graph(got, g)
    assert got["graph_timings"]["edges_s"] > 0 and got["graph_timings"]["gfa_s"] > 0


# ------------------------------------------------------------------ 6. k = 15, 1 GiB ---------------
TILE = 4096                                                  # addresses of one compaction tile of kmer_unitig.hip


def test_targets_at_the_ends_of_the_range_k15(gpu):
    """One 1 GiB table: every canonical address of one 4096-address tile is a node with one predecessor shared among four of
    them, so each is the target of an edge (more than 3 * 256 in the tile); and two predecessors each for a node below 4096 and
    for the highest canonical address TTTTTTTCAAAAAAA, which makes both of them targets too."""
    k = 15
    first, last = ref.encode("A" * 9 + "CGTACG"), ref.encode("TTTTTTTCAAAAAAA")
    assert first < TILE and first == ref.canon(first, k) and last == ref.canon(last, k)
    assert all(ref.canon(x, k) != x for x in range(last + 1, last + 50))
    tile0 = ref.encode("ACGTTGCAC" + "A" * 6)
    assert tile0 % TILE == 0
    crowd = [x for x in range(tile0, tile0 + TILE) if x == ref.canon(x, k)]
    nodes = set(crowd) | {first, last}
    nodes |= {ref.canon((1 << (2 * (k - 1))) | (x >> 2), k) for x in crowd}                     # C + the first k - 1 letters
    for x in (first, last):
        nodes |= {ref.canon((b << (2 * (k - 1))) | (x >> 2), k) for b in (1, 2)}                # C and G in front
    counts = {x: 1 + x % 3 for x in nodes}
    want = ref.expected(counts, k)
    g = gref.graph(want)
    row_of = {int(a): r for r, a in enumerate(want["first_addr"])}
    targets = set(g["edge_to"].tolist())
    assert sum(1 for x in crowd if want["n_kmers"][row_of[x]] == 1 and row_of[x] in targets) > 3 * 256
    assert row_of[first] in targets and row_of[last] in targets and want["n_kmers"][row_of[last]] == 1
    table = np.zeros(4 ** k, dtype=np.uint8)
    table[np.fromiter(counts.keys(), dtype=np.int64)] = np.fromiter(counts.values(), dtype=np.uint8)
    with gs.Device([table]) as dev:
        got = graph_at(dev.ptrs[0], k)
    same(got, want)
    same_graph(got, g)


# ------------------------------------------------------------------ 7. k = 17 ----------------------
K17_SEED = 1701                                              # the first seed from 1700 on whose edges cross as crosses() asks


def k17_sequences(seed):
    k = 17
    rng, seen = random.Random(seed), set()
    seqs = []
    for _ in range(2):                                       # two Ys: a stem that forks into two arms
        stem, arm1, arm2 = (ui.distinct_sequence(rng, 60, k, seen) for _ in range(3))
        seqs += [stem + arm1, stem[-(k - 1):] + arm2]
    return seqs


def crosses(want, g, k=17):
    """An edge from a head whose node lies below 2^32 to a tail whose node lies at or above 2^33, and one the other way."""
    up = down = False
    for r, s, q, u, _ in g["edges"]:
        h = ref.canon(gref.head(want["paths"][r], s, k), k)
        t = ref.canon(want["paths"][q][-1] if u else want["paths"][q][0], k)
        up |= h < 2 ** 32 and t >= 2 ** 33
        down |= h >= 2 ** 33 and t < 2 ** 32
    return up and down


def test_addresses_beyond_32_bits_k17(gpu):
    """A 16 GiB table counted on the GPU and never left HBM, with a few hundred nodes in two Y branches: edges whose head and
    whose target lie on either side of 2^32 and 2^33."""
    k = 17
    seqs = k17_sequences(K17_SEED)
    counts = {}
    for s in seqs:                                           # as the indexer counts them: a k-mer that two sequences share counts twice
        for x in ref.kmers_of(s, k):
            counts[x] = counts.get(x, 0) + 1
    want = ref.expected(counts, k)
    g = gref.graph(want)
    assert 200 <= want["n_nodes"] <= 500 and want["n_branching"] == 2 and g["n_edges"] == 8 and crosses(want, g)
    text = "".join(f">s{i}\n{s}\n" for i, s in enumerate(seqs)).encode("ascii")
    with gs.lib().Indexer(k, device=0) as ix:
        ix.feed(text)
        fin = ix.finish()
        assert fin["num_kmers"] == sum(len(s) - k + 1 for s in seqs) == sum(counts.values()) == int(want["depth"].sum())
        got = graph_at(ix.table_device_ptr(), k)
    same(got, want)
    same_graph(got, g)


# ------------------------------------------------------------------ 8. slices and state ------------
def test_slices_and_state(gpu):
    k = 7
    counts, want, g = edge_cases(k)["random 0.3"]
    cut = ref.expected(counts, k, 2, 255)
    g_cut = gref.graph(cut)
    assert g["n_edges"] > 0 and g_cut["gfa"] != g["gfa"] and len(g["gfa"]) >= 3
    s_end = g["gfa"].index(b"\nL\t") + 1                      # where the L-lines begin
    lib = gs.lib()
    with gs.Device([ref.table_of(counts, k)]) as dev, lib.Unitigs(k, device=0) as u:
        plain = read_out(u, u.build(dev.ptrs[0], 1, 255, 1))  # no graph() call: what a build gives today
        same(plain, want)
        raw = lib.load()
        assert raw.pk_unitig_edges(u._h, None, None, None, 0) == lib.PK_ERR_STATE and raw.pk_unitig_gfa_text(u._h, None, 0, 0) == lib.PK_ERR_STATE
        got = read_graph(u, plain)
        same_graph(got, g)
        assert u.gfa_text(0, 0).size == 0
        assert u.gfa_text(1, len(g["gfa"]) - 2).tobytes() == g["gfa"][1:-1]
        assert u.gfa_text(s_end - 9, 18).tobytes() == g["gfa"][s_end - 9:s_end + 9]
        for off, n in ((len(g["gfa"]) + 1, 0), (1, len(g["gfa"]))):
            with pytest.raises(ValueError, match="outside"):
                u.gfa_text(off, n)
        same(read_out(u, u.build(dev.ptrs[0], 2, 255, 1)), cut)          # another window: the graph is the old build's no more
        for call in (u.edges, u.gfa_text):
            with pytest.raises(lib.PkError) as exc:
                call()
            assert exc.value.code == lib.PK_ERR_STATE
        same_graph(read_graph(u, {}), g_cut)
        same_graph(read_graph(u, {}), g_cut)                 # and again on the same build


# ------------------------------------------------------------------ 9. the CLI ---------------------
def test_cli_gfa(gpu, tmp_path):
    """indexer.py on a small FASTA, unitigs.py --gfa on its table: the four files, S-lines that hold the FASTA records, L-lines
    that overlap by k - 1 letters across a node, and as many of them as the count identity gives on the table."""
    k = 9
    fa = tmp_path / "g.fa"
    fa.write_bytes(bytes(synth.family(0, 20_000)[0]))
    gs.run_py("indexer.py", str(fa), "g", str(k), cwd=str(tmp_path))
    kin = f"{fa}.{k:02d}.kin"
    table = np.fromfile(kin, dtype=np.uint8)
    r = gs.run_py("unitigs.py", "u", kin, "--min-count", "2", "--max-count", "200", "--gfa", cwd=str(tmp_path))
    assert sorted(p.name for p in tmp_path.glob("u.*")) == ["u.kmu", "u.kmu.json", "u.unitigs.fa", "u.unitigs.gfa"]
    meta, kmu = json.load(open(tmp_path / "u.kmu.json")), np.load(tmp_path / "u.kmu")
    last = r.stdout.strip().splitlines()[-1]
    assert last.endswith(f"u.unitigs.fa, {meta['n_edges']} edges in u.unitigs.gfa"), last
    parsed = gref.parse_gfa((tmp_path / "u.unitigs.gfa").read_bytes())
    fasta = (tmp_path / "u.unitigs.fa").read_bytes().decode("ascii").split("\n")
    assert [s[1] for s in parsed["segments"]] == fasta[1:-1:2] and [">" + s[0] for s in parsed["segments"]] == fasta[0:-1:2]
    assert [s[3] for s in parsed["segments"]] == kmu["depth"].tolist() and [s[2] for s in parsed["segments"]] == (kmu["n_kmers"] + np.uint64(k - 1)).tolist()
    # the nodes and their degrees with numpy: member[o] for every oriented k-mer o
    x = np.arange(4 ** k, dtype=np.int64)
    rc, rest = np.zeros_like(x), x.copy()
    for _ in range(k):
        rc = (rc << 2) | (3 - (rest & 3))
        rest >>= 2
    member = (table[np.minimum(x, rc)] >= 2) & (table[np.minimum(x, rc)] <= 200)
    degree = sum(member[((x << 2) | b) & (4 ** k - 1)].astype(np.int64) for b in range(4))
    n_edges = int(degree[member].sum()) - 2 * int((kmu["n_kmers"].astype(np.int64) - 1).sum())
    assert meta["n_edges"] == n_edges == len(parsed["links"]) == kmu["edge_from"].size > 0 and meta["edges_dropped"] == 0

    class Nodes:                                             # what check_overlaps asks of a graph
        pass
    Nodes.k, Nodes.oriented = k, set(np.flatnonzero(member).tolist())
    gref.check_overlaps(parsed, Nodes)
    assert [(e[0], e[2], e[1] | (e[3] << 1)) for e in parsed["links"]] == list(zip(kmu["edge_from"].tolist(), kmu["edge_to"].tolist(), kmu["edge_orient"].tolist()))
    r = gs.run_py("unitigs.py", "u", kin, "--gfa", cwd=str(tmp_path), status=1)          # no file is overwritten
    assert any(line.startswith("error: ") for line in r.stderr.splitlines())
