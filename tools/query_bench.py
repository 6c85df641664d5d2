"""Times the query path (kmer_query.hip) at k = 15 against N = 13 tables that lie in HBM, the query text in HBM too.

Two query shapes: the 800 Mbp synthetic genome of bench.py (synth.c2) and a read set of 400 000 records of 1 kbp
(synth.generate(34, 400_000_000, 400_000), as tools/reads_probe.py).  The tables are counted on the GPU from 13 members of
synth.family and copied to buffers of their own.  Per shape: one warm-up, then the median of 5 timed runs of
reset + feed_device + finish + results (wall clock around calls that block until the device is done), and the library's own
HIP-event times of the structure pass, the squeeze and the lookup kernels (pk_indexer_timings) of the last run.

    python tools/query_bench.py [out.json]     both shapes, then one `rocprofv3 --kernel-trace --stats` run of a child
                                               (`--once genome`), whose kernel stats go to profiles/query_genome_kernel_stats.csv
    python tools/query_bench.py --once SHAPE   warm-up + one run of one shape (what the profiled child runs)
    --bin W        the same inputs tallied in bins of W valid windows (pk_query_set_bins); the rows are fetched with
                   bin_results instead of results
    --coords       with --bin: the rows' base coordinates too (pk_query_set_coords, kmer_coords.hip), fetched with
                   bin_coords; `coords_s_runs` holds the coordinate kernels' HIP-event time of every timed run
    --spectrum     count spectra (pk_query_set_spectrum, DESIGN.md 4.10 "Count spectra"): per shape and kind of table the
                   lookup with the option off and on, per record and in bins of 10 000 and of 100 windows (with --bin W:
                   in bins of W only), the text uploaded and the tables staged once for all of them.  The kinds of table are
                   the 13 genome tables and 13 tables that are all zero (one count dominates).  The wall clock of a run
                   with the option on includes the download of the spectra (skipped, and said so, above
                   PK_QUERY_BENCH_MAX_DOWNLOAD bytes [16 GiB]); a configuration whose spectra do not fit the device is
                   recorded with the library's refusal.  Writes profiles/query_spectrum_k15_n13.json.
    --pairs        shared windows per pair of tables (pk_query_set_pairs, DESIGN.md 4.10 "Shared windows"): the matrix of
                   --spectrum with that option off and on, against the 13 genome tables only; the wall clock of a run with the
                   option on includes the download of the rows x 78 u64.  Writes profiles/query_pairs_k15_n13.json.
    --runs R       timed runs per shape [5]
    --no-trace     skip the rocprofv3 run
    PK_QUERY_BENCH_BP / PK_QUERY_BENCH_TABLE_BP scale the genome and the table genomes down for a rehearsal.

Writes profiles/query_k15_n13.json (or out.json).  `lookup_s_runs` holds the lookup kernels' HIP-event time of every timed
run, `front_s_runs` that of the structure pass and the squeeze together; profiles/query_bins_k15_n13.json and
profiles/query_coords_k15_n13.json were put together from such runs of two builds."""
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import synth  # noqa: E402
from pykmer_amd import _lib  # noqa: E402

K, N = 15, 13


def stage_tables(table_bp: int, zero: bool = False):
    """13 tables counted from the members of synth.family; zero: counted from nothing, so every count is 0."""
    bufs = []
    with _lib.Indexer(K) as ix:
        for i in range(N):
            ix.reset()
            if not zero:
                ix.feed(synth.family(i, table_bp)[0])
            ix.finish()
            b = _lib.DeviceBuffer(4 ** K)
            ix.table_slice_to_device(b.ptr, 0, 4 ** K)
            bufs.append(b)
    return bufs


def shapes(genome_bp: int):
    yield "genome", lambda: synth.c2(genome_bp, seed=2)
    yield "reads", lambda: synth.generate(34, genome_bp // 2, max(1, genome_bp // 2000))


def run_shape(make, ptrs, runs: int, bin_windows: int = None, coords: bool = False):
    fa, bp = make()
    text = _lib.DeviceBuffer(len(fa) + 64)
    text.upload(np.asarray(fa))
    try:
        with _lib.QueryIndexer(K) as q:
            times, lookups, fronts, coord_times = [], [], [], []
            for i in range(runs + 1):                                     # the first run warms up: allocations, code load
                q.reset()
                q.set_tables(ptrs, 1, 255)
                if bin_windows is not None:
                    q.set_bins(bin_windows)
                    if coords:
                        q.set_coords(True)
                t0 = time.perf_counter()
                q.feed_device(text.ptr, len(fa))
                fin = q.finish()
                if bin_windows is not None:
                    hits, depth, bin_first = q.bin_results(fin["n_records"])
                    if coords:
                        bin_start, bin_end = q.bin_coords()
                else:
                    hits, depth = q.results(fin["n_records"])
                if i:
                    times.append(time.perf_counter() - t0)
                    t = q.timings()                                        # a reset zeroes the library's timers
                    lookups.append(float(t["lookup_s"]))
                    fronts.append(float(t["scan_s"] + t["squeeze_s"]))
                    coord_times.append(float(t.get("coords_s", 0.0)))
            t = q.timings()
        med = statistics.median(times) if times else float("nan")
        front = t["scan_s"] + t["squeeze_s"]
        return {"bp": int(bp), "text_bytes": len(fa), "records": fin["n_records"], "windows": fin["num_kmers"], "tables": len(ptrs),
                "bin_windows": bin_windows, "coords": coords, "rows": int(hits.shape[0]), "runs": times, "lookup_s_runs": lookups,
                "front_s_runs": fronts, "coords_s_runs": coord_times,
                "coords_s_median": statistics.median(coord_times) if coord_times else float("nan"),
                "coords_span_of_row_0": [int(bin_start[0]), int(bin_end[0])] if coords and len(bin_start) else None,
                "lookup_s_median": statistics.median(lookups) if lookups else float("nan"), "median_s": med, "best_s": min(times) if times else med, "bp_per_s": bp / med,
                "lookups_per_s": fin["num_kmers"] * len(ptrs) / med,
                "device_s": {"structure_pass": t["scan_s"], "squeeze": t["squeeze_s"], "lookup_kernels": t["lookup_s"],
                             "coords_kernels": float(t.get("coords_s", 0.0))},
                "coords_over_structure_plus_squeeze": float(t.get("coords_s", 0.0)) / front,
                "lookup_share_of_device_time": t["lookup_s"] / (front + t["lookup_s"]),
                "lookup_over_structure_plus_squeeze": t["lookup_s"] / front,
                "lookups_per_s_kernels_only": fin["num_kmers"] * len(ptrs) / t["lookup_s"],
                "hit_fraction_table0": float(hits[:, 0].sum()) / max(1, fin["num_kmers"])}
    finally:
        text.free()


def time_config(q, text, n_bytes: int, ptrs, runs: int, bin_windows, spectrum: bool, max_download: int, pairs: bool = False) -> dict:
    """1 warm-up + `runs` timed runs of one configuration on an indexer that other configurations have used before."""
    walls, lookups, rows, download = [], [], 0, None
    try:
        for i in range(runs + 1):
            q.reset()
            q.set_tables(ptrs, 1, 255)
            if bin_windows is not None:
                q.set_bins(bin_windows)
            if spectrum:
                q.set_spectrum(True)
            if pairs:
                q.set_pairs(True)
            t0 = time.perf_counter()
            q.feed_device(text.ptr, n_bytes)
            fin = q.finish()
            if bin_windows is not None:
                hits, depth, bin_first = q.bin_results(fin["n_records"])
            else:
                hits, depth = q.results(fin["n_records"])
            rows = int(hits.shape[0])
            spec_bytes = rows * len(ptrs) * 2048
            if spectrum:
                download = spec_bytes <= max_download
                if download:
                    spec = q.spectrum(rows)
                    if i == 0:                               # once per configuration: the identities of the definition
                        sums = spec.sum(axis=2, dtype=np.uint64)
                        assert (sums == sums[:, :1]).all() and int(sums[:, 0].sum()) == fin["num_kmers"], "spectra do not sum to the windows"
                        assert np.array_equal(spec[:, :, 1:].sum(axis=2, dtype=np.uint64), hits), "window 1-255 of the spectra is not the hits"
                    del spec
            if pairs:
                n_pairs = len(ptrs) * (len(ptrs) - 1) // 2
                download = rows * n_pairs * 8 <= max_download
                if download:
                    shared = q.pairs(rows)
                    if i == 0:                               # once per configuration: the bound of the definition
                        at = 0
                        for a in range(len(ptrs)):
                            for b in range(a + 1, len(ptrs)):
                                assert (shared[:, at] <= np.minimum(hits[:, a], hits[:, b])).all(), "a pair shares more than its tables hit"
                                at += 1
                        pair_sum = int(shared.sum(dtype=np.uint64))
                    del shared
            if i:
                walls.append(time.perf_counter() - t0)
                lookups.append(float(q.timings()["lookup_s"]))
    except _lib.PkError as exc:
        return {"bin_windows": bin_windows, "spectrum": spectrum, "pairs": pairs, "refused": str(exc)}
    if pairs:
        return {"bin_windows": bin_windows, "pairs": True, "rows": rows, "pairs_bytes": rows * len(ptrs) * (len(ptrs) - 1) // 2 * 8,
                "downloaded": download, "shared_sum": pair_sum if download else None, "lookup_s_runs": lookups,
                "lookup_s_median": statistics.median(lookups), "lookup_s_min": min(lookups), "lookup_s_max": max(lookups), "wall_s_runs": walls,
                "wall_s_median": statistics.median(walls)}
    return {"bin_windows": bin_windows, "spectrum": spectrum, "rows": rows, "spectrum_bytes": rows * len(ptrs) * 2048 if spectrum else 0,
            "downloaded": download, "lookup_s_runs": lookups, "lookup_s_median": statistics.median(lookups), "lookup_s_min": min(lookups),
            "lookup_s_max": max(lookups), "wall_s_runs": walls, "wall_s_median": statistics.median(walls)}


def run_spectrum_matrix(genome_bp: int, table_bp: int, runs: int, bins, path: str, pairs: bool = False) -> dict:
    """The option (count spectra; pairs: shared windows) off and on, per kind of table, shape and bin size."""
    max_download = int(os.environ.get("PK_QUERY_BENCH_MAX_DOWNLOAD", 16 << 30))
    out = {"k": K, "n_tables": N, "table_genome_bp": table_bp, "runs": runs,
           "option": "pairs" if pairs else "spectrum",
           "method": f"per configuration 1 warm-up + {runs} runs of reset/set_*/feed_device/finish/results[/spectrum|pairs]; lookup_s from HIP events "
                     "(pk_indexer_timings), wall_s around the blocking calls, the download of the option's array included where `downloaded`",
           "on_over_off": "lookup_s_median with the option on over the one with it off, same bins, same tables, same build"}
    texts = {}
    for name, make in shapes(genome_bp):
        fa, bp = make()
        buf = _lib.DeviceBuffer(len(fa) + 64)
        buf.upload(np.asarray(fa))
        texts[name] = (buf, len(fa), int(bp))
        del fa
    for kind in ("genome_tables",) if pairs else ("genome_tables", "zero_tables"):
        bufs = stage_tables(table_bp, zero=kind == "zero_tables")
        ptrs = [b.ptr for b in bufs]
        out[kind] = {}
        for name, (buf, n_bytes, bp) in texts.items():
            res = out[kind][name] = {"bp": bp, "text_bytes": n_bytes, "configs": []}
            with _lib.QueryIndexer(K) as q:
                for W in bins:
                    off = time_config(q, buf, n_bytes, ptrs, runs, W, False, max_download)
                    on = time_config(q, buf, n_bytes, ptrs, runs, W, not pairs, max_download, pairs=pairs)
                    if "refused" not in on and "refused" not in off:
                        on["on_over_off"] = on["lookup_s_median"] / off["lookup_s_median"]
                    res["configs"] += [off, on]
                    print(kind, name, json.dumps(off), json.dumps(on), flush=True)
            with open(path + ".tmp", "w") as fh:             # what is measured so far survives a run that is cut short
                json.dump(out, fh, indent=1)
            os.replace(path + ".tmp", path)
        for b in bufs:
            b.free()
    for buf, _, _ in texts.values():
        buf.free()
    return out


def kernel_stats(argv, dest):
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    d = tempfile.mkdtemp(prefix="qprof")
    subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "q", "--"] + argv, check=True, timeout=1500, cwd=ROOT)
    path = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
    with open(path) as fh:
        rows = list(csv.DictReader(fh))
    shutil.copy(path, dest)
    shutil.rmtree(d, ignore_errors=True)
    return rows


def main():
    argv, args, opts = sys.argv[1:], [], {"--bin": None, "--runs": 5}
    while argv:
        a = argv.pop(0)
        if a in opts:
            opts[a] = int(argv.pop(0))
        elif not a.startswith("--"):
            args.append(a)
    bin_windows, runs = opts["--bin"], opts["--runs"]
    coords = "--coords" in sys.argv
    if coords and bin_windows is None:
        sys.exit("error: --coords needs --bin W")
    genome_bp = int(os.environ.get("PK_QUERY_BENCH_BP", 800_000_000))
    table_bp = int(os.environ.get("PK_QUERY_BENCH_TABLE_BP", 40_000_000))
    if "--spectrum" in sys.argv or "--pairs" in sys.argv:
        pairs = "--pairs" in sys.argv
        path = args[0] if args else os.path.join(ROOT, "profiles", "query_pairs_k15_n13.json" if pairs else "query_spectrum_k15_n13.json")
        run_spectrum_matrix(genome_bp, table_bp, runs, [bin_windows] if bin_windows is not None else [None, 10_000, 100], path, pairs=pairs)
        return
    bufs = stage_tables(table_bp)
    ptrs = [b.ptr for b in bufs]
    if "--once" in sys.argv:
        run_shape(dict(shapes(genome_bp))[args[0]], ptrs, 1, bin_windows, coords)
        return
    out = {"k": K, "n_tables": N, "table_genome_bp": table_bp, "layout": "one 4^k-byte table per sample (not interleaved)",
           "bin_windows": bin_windows, "coords": coords,
           "method": f"1 warm-up + median of {runs} runs of reset/feed_device/finish/results; device_s from HIP events (pk_indexer_timings)"}
    for name, make in shapes(genome_bp):
        out[name] = run_shape(make, ptrs, runs, bin_windows, coords)
        print(name, json.dumps(out[name]), flush=True)
    for b in bufs:
        b.free()
    if "--no-trace" not in sys.argv:
        once = [sys.executable, os.path.abspath(__file__), "--once", "genome"] + (["--bin", str(bin_windows)] if bin_windows is not None else []) + (["--coords"] if coords else [])
        rows = kernel_stats(once, os.path.join(ROOT, "profiles", "query_genome_kernel_stats.csv"))
        out["genome_kernel_trace_ms_per_call"] = {r["Name"].split("(")[0][:60]: round(float(r["AverageNs"]) / 1e6, 4) for r in rows
                                                   if "k_query" in r["Name"] or "k_squeeze" in r["Name"] or "k_coords" in r["Name"]}
    path = args[0] if args else os.path.join(ROOT, "profiles", "query_coords_k15_n13.json" if coords else "query_k15_n13.json")
    with open(path + ".tmp", "w") as fh:
        json.dump(out, fh, indent=1)
    os.replace(path + ".tmp", path)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
