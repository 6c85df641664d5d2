"""Times pk_unitig_build (kmer_unitig.hip) on three tables that lie in HBM, window 1..255, --min-kmers 1:

  genome_k17   the k = 17 table of synth.c2(100 Mbp, seed 2), the first eighth of the benchmark's genome size: long unitigs,
               few branches
  genome_k15   the k = 15 table of synth.c2(800 Mbp, seed 2), the benchmark's genome: about half of all addresses are nodes
               and nearly every unitig is one k-mer -- the tangled worst case of the link pass
  markers_k15  `extract.py --table max` over the 7 present + 6 absent tables of tools/extract_bench.py (synth.family(i, 40 Mbp)):
               the intended use

Per table, in one process: one warm-up build, then `--runs` (3) timed builds with a fresh builder each; links_s, paths_s and
cycles_s are the library's HIP-event seconds (pk_unitig_timings: the kernels between two events on the builder's stream, the
allocations and the read-backs of the counts outside them); the medians are reported with every run beside them.  Beside them
hipMemcpyDtoDAsync of the table between two HIP events on the null stream (the floor of a dense pass, as tools/filter_bench.py
times it) and pk_extract_device counting the same window on the same table (count + scan, no arrays), one warm-up and the
median of the same number of runs each.

    python tools/unitig_bench.py [out.json] [--runs R] [--only NAME] [--gfa]
    --gfa also runs pk_unitig_graph behind every build and reports edges_s and gfa_s (pk_unitig_graph_timings), the edge totals
    and the GFA bytes beside links_s + paths_s + cycles_s of the same runs; it writes profiles/unitigs_gfa.json instead.
    PK_UNITIG_BENCH_SCALE=0.01 scales the three genomes down for a rehearsal.

Writes profiles/unitigs.json (profiles/unitigs_gfa.json with --gfa), or out.json."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import filter_bench  # noqa: E402
import synth  # noqa: E402
from pykmer_amd import _lib  # noqa: E402

P, A = 7, 6


def time_table(name: str, ptr: int, k: int, hip, runs: int, gfa: bool = False) -> dict:
    n = 4 ** k
    builds, graphs, graph_totals = [], [], {}
    for i in range(runs + 1):
        with _lib.Unitigs(k) as u:
            totals = u.build(ptr, 1, 255, 1)
            if gfa:
                graph_totals = u.graph()
            if i:
                builds.append(u.timings())
                graphs.append(u.graph_timings() if gfa else {})
            else:
                n_kmers = u.rows()["n_kmers"]
        print(name, "build", i, dict(builds[-1], **graphs[-1]) if builds else "warm-up", flush=True)
    counts = []
    for i in range(runs + 1):
        m, _, s = _lib.extract_device([ptr], 1, n, 0, 1, 255, 1, 0)
        assert m >= totals["n_nodes"], (m, totals["n_nodes"])        # the window count sees non-canonical addresses too: there are none
        if i:
            counts.append(s)
    scratch = _lib.DeviceBuffer(n)
    try:
        copies = filter_bench.time_copy(hip, scratch.ptr, ptr, n, runs)
    finally:
        scratch.free()
    med = {key: statistics.median(b[key] for b in builds) for key in ("links_s", "paths_s", "cycles_s")}
    by_n = np.bincount(n_kmers.astype(np.int64))            # unitigs per n_kmers: half a billion rows are not sorted
    sizes = np.flatnonzero(by_n)[::-1]                       # descending
    bases_at = by_n[sizes] * (sizes + k - 1)
    bases = int(bases_at.sum())
    n50 = int(sizes[np.searchsorted(np.cumsum(bases_at), (bases + 1) // 2)] + k - 1) if sizes.size else 0
    top = np.repeat(sizes[:8], by_n[sizes[:8]])[:8]
    copy, count = statistics.median(copies), statistics.median(counts)
    graph = {}
    if gfa:                                                  # beside the three phases of the same runs
        build_s = [b["links_s"] + b["paths_s"] + b["cycles_s"] for b in builds]
        graph = {**graph_totals, "edges_s_runs": [g["edges_s"] for g in graphs], "gfa_s_runs": [g["gfa_s"] for g in graphs], "build_s_runs": build_s,
                 "edges_s_median": statistics.median(g["edges_s"] for g in graphs), "gfa_s_median": statistics.median(g["gfa_s"] for g in graphs),
                 "build_s_median": statistics.median(build_s)}
        graph["edges_over_build"] = graph["edges_s_median"] / graph["build_s_median"]
        graph["gfa_over_build"] = graph["gfa_s_median"] / graph["build_s_median"]
        graph["edges_over_copy"] = graph["edges_s_median"] / copy
    return {**graph, "kmer_len": k, "table_bytes": n, **totals, "n_unitigs": totals["n_linear"] + totals["n_circular"], "longest_bases": totals["longest_kmers"] + k - 1,
            "n50": n50, "bases": bases, "largest_n_kmers": [int(v) for v in top],
            "links_s_runs": [b["links_s"] for b in builds], "paths_s_runs": [b["paths_s"] for b in builds], "cycles_s_runs": [b["cycles_s"] for b in builds],
            "links_s_median": med["links_s"], "paths_s_median": med["paths_s"], "cycles_s_median": med["cycles_s"],
            "copy_s_runs": copies, "copy_s_median": copy, "extract_count_s_runs": counts, "extract_count_s_median": count,
            "links_over_copy": med["links_s"] / copy, "links_over_extract_count": med["links_s"] / count,
            "link_loads_per_node_bound": 16, "nodes_per_links_s": totals["n_nodes"] / med["links_s"] if med["links_s"] else None}


def counted(k: int, text):
    """An indexer whose table holds the k-mers of `text`; the table stays in HBM while the indexer lives."""
    ix = _lib.Indexer(k)
    ix.feed(text)
    ix.finish()
    return ix


def main():
    argv, args, runs, only, gfa = sys.argv[1:], [], 3, None, False
    while argv:
        a = argv.pop(0)
        if a == "--runs":
            runs = int(argv.pop(0))
        elif a == "--only":
            only = argv.pop(0)
        elif a == "--gfa":
            gfa = True
        elif not a.startswith("--"):
            args.append(a)
    scale = float(os.environ.get("PK_UNITIG_BENCH_SCALE", "1"))
    if _lib.device_count() < 1:
        sys.exit("error: unitig_bench.py needs a GPU")
    hip = filter_bench.hip_runtime()
    out = {"runs": runs, "scale": scale, "window": [1, 255], "min_kmers": 1,
           "method": f"per table 1 warm-up + median of {runs} builds with a fresh builder each, one process, tables resident in HBM; links_s, paths_s, "
                     "cycles_s from HIP events on the builder's stream around the kernels of each phase (pk_unitig_timings; allocations and the "
                     "read-backs of the counts lie outside the events); copy_s: hipMemcpyDtoDAsync of the table between two HIP events; "
                     "extract_count_s: pk_extract_device with cap = 0 on the same table and window (its own HIP events)"}
    if gfa:
        out["method"] += ("; --gfa: pk_unitig_graph behind every build, the warm-up too; edges_s (end map, count, scan, fill) and gfa_s (line sizes, "
                          "scans, S- and L-lines) from HIP events on the same stream (pk_unitig_graph_timings), their allocations and read-backs "
                          "outside; build_s = links_s + paths_s + cycles_s of the same run")
    path = args[0] if args else os.path.join(ROOT, "profiles", "unitigs_gfa.json" if gfa else "unitigs.json")

    def done(name, result):
        out[name] = result
        print(name, json.dumps(result), flush=True)
        with open(path + ".tmp", "w") as fh:                 # after every table: a later one that fails leaves the earlier figures
            json.dump(out, fh, indent=1)
        os.replace(path + ".tmp", path)

    if only in (None, "genome_k17"):
        with counted(17, synth.c2(int(100_000_000 * scale), seed=2)[0]) as ix:
            done("genome_k17", time_table("genome_k17", ix.table_device_ptr(), 17, hip, runs, gfa))
    if only in (None, "markers_k15"):
        n = 4 ** 15
        bufs, marker, hist = [], _lib.DeviceBuffer(n), _lib.DeviceBuffer(256 * 8)
        try:
            with _lib.Indexer(15) as ix:
                for i in range(P + A):
                    ix.reset()
                    ix.feed(synth.family(i, int(40_000_000 * scale))[0])
                    ix.finish()
                    bufs.append(_lib.DeviceBuffer(n))
                    ix.table_slice_to_device(bufs[-1].ptr, 0, n)
            hist.zero()
            _lib.extract_table_device([b.ptr for b in bufs], P, n, 1, 255, P, 0, "max", marker.ptr, hist.ptr)
            for b in bufs:
                b.free()
            bufs = []
            done("markers_k15", time_table("markers_k15", marker.ptr, 15, hip, runs, gfa))
        finally:
            for b in bufs + [marker, hist]:
                b.free()
    if only in (None, "genome_k15"):
        with counted(15, synth.c2(int(800_000_000 * scale), seed=2)[0]) as ix:
            done("genome_k15", time_table("genome_k15", ix.table_device_ptr(), 15, hip, runs, gfa))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
