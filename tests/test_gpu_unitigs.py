"""pk_unitig and unitigs.py on the GPU against tests/unitig_ref.py: the FASTA bytes, the four row arrays and the totals are
compared for equality.  Every test first asserts on the reference output that its input holds the feature it is named for."""
import functools
import random

import numpy as np
import pytest

import gpu_support as gs
import synth
import unitig_inputs as ui
import unitig_ref as ref
from unitig_support import build_at, check, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    return gs.lib()


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
    return {name: (c, ref.expected(c, k)) for name, c in cases.items()}


def test_edge_cases_hold_every_rule():
    """The precondition of test_every_edge_rule, on the reference alone: a self-loop, a hairpin, a double edge, a 2-cycle and
    a longer cycle whose smallest address is not the table's lowest node, and linear unitigs of more than one k-mer.  The
    double edge is two edges between two nodes, o -> t and t -> o: one o with the successors t and rc(t) cannot exist for an
    odd k (unitig_inputs.features proves and asserts it)."""
    found = set()
    for k in (5, 7):
        for name, (counts, want) in edge_cases(k).items():
            found |= ui.features(want["graph"])
            rings = want["n_kmers"][want["circular"] == 1]
            found |= {"2-cycle"} if (rings == 2).any() else set()
            if (rings > 2).any() and int(want["first_addr"][want["circular"] == 1][0]) > min(want["graph"].S):
                found.add("long cycle")
            if ((want["circular"] == 0) & (want["n_kmers"] >= 3)).any():
                found.add("path")
            if name == "random 1.0":
                assert want["n_nodes"] == want["n_branching"] == 4 ** k // 2 == len(want["n_kmers"])
    assert found == {"self_loop", "hairpin", "double_edge", "2-cycle", "long cycle", "path"}, found


@pytest.mark.parametrize("k", [5, 7])
def test_every_edge_rule(gpu, k):
    for name, (counts, want) in edge_cases(k).items():
        check(counts, k, want=want)


# ------------------------------------------------------------------ 2. window and depth ------------
@pytest.mark.parametrize("beside", [0, 2, 3, 250, 251, 255])
def test_window_and_depth(gpu, beside):
    """A path of 300 nodes of count 250 under the window 3-250, and two k-mers beside it -- a second successor of one node, a
    second predecessor of another -- with the count `beside`: outside the window they neither join nor branch, inside it they
    cut the path in three.  depth sums the raw bytes: 300 * 250 > 2^16."""
    k, mn, mx = 7, 3, 250
    rng, seen = random.Random(77), set()
    path = ui.distinct_sequence(rng, 300 + k - 1, k, seen)
    counts = ui.counts_of([path], k, 250)
    assert len(counts) == 300
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
    inside = mn <= beside <= mx
    assert want["n_nodes"] == (302 if inside else 300)
    if inside:
        assert len(want["n_kmers"]) >= 4 and want["n_branching"] >= 2 and want["longest_kmers"] < 300
    else:
        assert want["n_kmers"].tolist() == [300] and want["depth"].tolist() == [75000] and want["n_branching"] == 0
    check(counts, k, mn, mx, want=want)


# ------------------------------------------------------------------ 3. --min-kmers -----------------
def test_min_kmers(gpu):
    """M = 1, 2 and n_max + 1 on paths of 1, 1, 2, 5 and 30 k-mers and rings of 2 and 12: dropped unitigs get no row and are not
    reported as cycles, the rows are numbered anew, and n_short / nodes_short hold what was dropped."""
    k = 7
    rng, seen = random.Random(91), set()
    seqs = [ui.distinct_sequence(rng, n + k - 1, k, seen) for n in (1, 1, 2, 5, 30)]
    seqs += [ui.distinct_sequence(rng, n, k, seen, circular=True) for n in (2, 12)]
    counts = ui.counts_of(seqs, k, 3)
    full = ref.expected(counts, k)
    assert sorted(full["n_kmers"].tolist()) == [1, 1, 2, 2, 5, 12, 30] and full["n_circular"] == 2 and full["n_nodes"] == 53
    for M, rows, short, nodes_short in ((1, 7, 0, 0), (2, 5, 2, 2), (3, 3, 4, 6), (31, 0, 7, 53)):
        want = ref.expected(counts, k, 1, 255, M)
        assert (len(want["n_kmers"]), want["n_short"], want["nodes_short"]) == (rows, short, nodes_short), M
        assert want["n_circular"] == (2 if M <= 2 else 1 if M == 3 else 0)
        got, _ = check(counts, k, M=M, want=want)
        assert got["bytes"] == len(want["fasta"]) and (rows or got["fasta"] == b"")


# ------------------------------------------------------------------ 4. scale seams at k = 15 -------
TILE = 4096                                                  # addresses of one compaction tile of kmer_unitig.hip


def test_scale_seams_k15(gpu):
    """One 1 GiB table: a unitig of more than 70 000 k-mers (one lane's long loop, past any 16-bit counter), more than 1001
    unitigs (the decimal row index grows at 10, 100 and 1000), more than 3 * 256 ends in one compaction tile, ends in the
    first tile and in the last tile that holds a canonical address (no address above TTTTTTTCAAAAAAA is canonical, so the last
    4096 addresses of the range hold no node), and a ring of 5 000 nodes that is one circular row.  The step bound is not
    reached: the build succeeds."""
    k = 15
    rng, seen = random.Random(1500), set()
    first, last = ref.encode("A" * 9 + "CGTACG"), ref.encode("TTTTTTTCAAAAAAA")
    assert first < TILE and first == ref.canon(first, k) and last == ref.canon(last, k)
    assert all(ref.canon(x, k) != x for x in range(last + 1, last + 50)) and ref.rc(last, k) > last
    tile0 = ref.encode("ACGTTGCAC" + "A" * 6)
    assert tile0 % TILE == 0
    crowd = [x for x in range(tile0, tile0 + TILE, 3) if x == ref.canon(x, k)][:900]
    singles = [first, last] + crowd
    for x in singles:
        text = list(ref.decode(x, k))
        seen.update(c for c in (ui._canon_at(text, 0, k - 1), ui._canon_at(text, 1, k - 1)) if c is not None)
    seqs = [ui.distinct_sequence(rng, 70_100, k, seen), ui.distinct_sequence(rng, 5_000, k, seen, circular=True)]
    seqs += [ui.distinct_sequence(rng, rng.randrange(k, 3 * k), k, seen) for _ in range(150)]
    counts = ui.counts_of(seqs, k, 2)
    counts.update({x: 1 for x in singles})
    want = ref.expected(counts, k)
    assert want["longest_kmers"] >= 70_000 and len(want["n_kmers"]) >= 1001
    rings = want["circular"] == 1
    assert rings.sum() == 1 and want["n_kmers"][rings].tolist() == [5000]
    ends = set()
    for path in want["paths"][:want["n_linear"]]:
        ends |= {ref.canon(path[0], k), ref.canon(path[-1], k)}
    assert sum(tile0 <= x < tile0 + TILE for x in ends) >= 3 * 256 and first in ends and last in ends
    assert b"\n>9\n" in want["fasta"] and b"\n>10\n" in want["fasta"] and b"\n>100\n" in want["fasta"] and b"\n>1000\n" in want["fasta"]
    table = np.zeros(4 ** k, dtype=np.uint8)
    table[np.fromiter(counts.keys(), dtype=np.int64)] = np.fromiter(counts.values(), dtype=np.uint8)
    with gs.Device([table]) as dev:
        got = build_at(dev.ptrs[0], k)
    same(got, want)
    assert got["timings"]["links_s"] > 0 and got["timings"]["paths_s"] > 0 and got["timings"]["cycles_s"] > 0


# ------------------------------------------------------------------ 5. 64-bit addresses at k = 17 --
def test_addresses_beyond_32_bits_k17(gpu):
    """A 16 GiB table counted on the GPU and never left HBM, with a few hundred nodes: paths whose successive addresses cross
    2^32 and 2^33, and nodes above 2^33."""
    k = 17
    rng, seen = random.Random(1700), set()
    seqs = [ui.distinct_sequence(rng, n, k, seen) for n in (150, 90, 40, 17)] + [ui.distinct_sequence(rng, 30, k, seen, circular=True)]
    counts = ui.counts_of(seqs, k, 1)
    want = ref.expected(counts, k)
    assert 200 <= want["n_nodes"] <= 400 and want["n_circular"] == 1 and want["n_linear"] == 4
    steps = [(ref.canon(a, k), ref.canon(b, k)) for path in want["paths"] for a, b in zip(path, path[1:])]
    for border in (2 ** 32, 2 ** 33):
        assert any(min(a, b) < border <= max(a, b) for a, b in steps), border
    assert max(counts) >= 2 ** 33
    text = "".join(f">s{i}\n{s}\n" for i, s in enumerate(seqs)).encode("ascii")
    with gs.lib().Indexer(k, device=0) as ix:
        ix.feed(text)
        fin = ix.finish()
        assert fin["num_kmers"] == sum(len(s) - k + 1 for s in seqs) == want["n_nodes"]
        got = build_at(ix.table_device_ptr(), k)
    same(got, want)


def test_build_unitigs_on_a_resident_table(gpu):
    """pykmer_amd.unitigs.build_unitigs on a table that lies in HBM already: nothing is staged, the bytes come back."""
    from pykmer_amd import staging, unitigs
    k = 7
    counts, want = edge_cases(k)["ring"][0], ref.expected(edge_cases(k)["ring"][0], k, 1, 255, 2)
    assert want["n_circular"] == 1 and want["n_linear"] >= 1
    with gs.Device([ref.table_of(counts, k)]) as dev:
        got = unitigs.build_unitigs(staging.ResidentTable(dev.ptrs[0], 4 ** k, 4 ** k), min_kmers=2)
        with pytest.raises(ValueError, match="window 200-255"):
            unitigs.build_unitigs(staging.ResidentTable(dev.ptrs[0], 4 ** k, 4 ** k), min_count=200)
    assert got["fasta"] == want["fasta"] and got["n_unitigs"] == len(want["n_kmers"]) and got["n_short"] == want["n_short"]
    for key in ("first_addr", "n_kmers", "depth", "circular"):
        assert np.array_equal(got[key], want[key]), key
    lengths = want["n_kmers"] + np.uint64(k - 1)
    assert (got["bases"], got["longest"], got["n50"]) == (int(lengths.sum()), int(lengths.max()), unitigs.n50(lengths))
    assert got["links_s"] > 0 and got["paths_s"] > 0


# ------------------------------------------------------------------ 6. the CLI, end to end ---------
def test_cli_end_to_end(gpu, tmp_path):
    """indexer.py on a small FASTA, unitigs.py on its table, indexer.py on the unitigs: the non-zero addresses of that table
    are exactly the input table's nodes in the window.  The loop closes without the reference module."""
    k = 9
    fa = tmp_path / "g.fa"
    fa.write_bytes(bytes(synth.family(0, 20_000)[0]))
    gs.run_py("indexer.py", str(fa), "g", str(k), cwd=str(tmp_path))
    table = np.fromfile(f"{fa}.{k:02d}.kin", dtype=np.uint8)
    assert table.size == 4 ** k
    nodes = np.flatnonzero((table >= 2) & (table <= 200))
    assert 100 < nodes.size < np.count_nonzero(table)
    r = gs.run_py("unitigs.py", "u", f"{fa}.{k:02d}.kin", "--min-count", "2", "--max-count", "200", cwd=str(tmp_path))
    last = r.stdout.strip().splitlines()[-1]
    assert f"from {nodes.size} k-mers" in last and last.endswith("u.unitigs.fa") and " unitigs (" in last, last
    assert sorted(p.name for p in tmp_path.glob("u.*")) == ["u.kmu", "u.kmu.json", "u.unitigs.fa"]
    kmu = np.load(tmp_path / "u.kmu")
    assert int(kmu["n_nodes"]) == nodes.size == int(kmu["n_kmers"].sum()) and int(kmu["depth"].sum()) == int(table[nodes].sum())
    gs.run_py("indexer.py", str(tmp_path / "u.unitigs.fa"), "again", str(k), cwd=str(tmp_path))
    again = np.fromfile(f"{tmp_path / 'u.unitigs.fa'}.{k:02d}.kin", dtype=np.uint8)
    assert np.array_equal(np.flatnonzero(again), nodes)
    r = gs.run_py("unitigs.py", "u", f"{fa}.{k:02d}.kin", cwd=str(tmp_path), status=1)          # no file is overwritten
    assert any(line.startswith("error: ") for line in r.stderr.splitlines())
