"""Times the two phases of mask.py (kmer_cover.hip, kmer_intervals.hip) on the inputs of tools/query_bench.py: k = 15, N = 13 tables counted from
synth.family, the 800 Mbp genome and the read set of 400 000 records of 1 kbp, text and tables in HBM.

Phase 1: the cover lookup (pk_query_set_cover: k_cover_scan + k_query_cover) beside the plain per-record lookup of the same
build in the same process (k_query_count + k_query_scan + k_query_lookup); both are `lookup_s` of pk_indexer_timings, HIP
events around the kernels behind the squeeze.  Phase 2: the apply kernel (pk_query_set_mask: `mask_s`, HIP events around
k_mask_apply) with the cover bits of phase 1, soft and hard, beside hipMemcpyDtoDAsync of the same text between two HIP events
on the null stream, as tools/filter_bench.py times the select.  Per configuration one warm-up, then the median of `--runs`
timed runs (5).  Once per shape the masked bases of phase 2 are checked against the set bits of phase 1.

    python tools/mask_bench.py [out.json] [--runs R]
    python tools/mask_bench.py --bed [out.json] [--runs R]
        the masked intervals (kmer_intervals.hip, pk_query_set_intervals) instead: in one process, per shape, the apply kernel
        alone (soft mask, intervals off) and the apply with the intervals on -- `mask_s` as above and the interval kernels'
        own HIP-event seconds (pk_query_interval_count: k_coords_sum + k_coords_scan + k_iv_count + k_iv_scan, and k_iv_write
        behind the read-back of the count) --, the number of intervals, and the device copy of the text.  The plain lookup is
        not timed.  Writes profiles/mask_bed_k15_n13.json.
    PK_QUERY_BENCH_BP / PK_QUERY_BENCH_TABLE_BP scale the genome and the table genomes down for a rehearsal.

Writes profiles/mask_k15_n13.json (or out.json)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import filter_bench  # noqa: E402
import query_bench  # noqa: E402
from pykmer_amd import _lib  # noqa: E402
from pykmer_amd.mask import count_bits  # noqa: E402

K = query_bench.K


def time_lookup(q, text, n_bytes: int, ptrs, runs: int, cover: bool):
    """lookup_s and scan_s + squeeze_s of 1 warm-up + `runs` runs; with `cover` also (bits, n_bases) of the last."""
    lookups, fronts, bits = [], [], None
    for i in range(runs + 1):
        q.reset()
        q.set_tables(ptrs, 1, 255)
        if cover:
            q.set_cover(True)
        q.feed_device(text.ptr, n_bytes)
        fin = q.finish()
        if i:
            t = q.timings()
            lookups.append(float(t["lookup_s"]))
            fronts.append(float(t["scan_s"] + t["squeeze_s"]))
    if cover:
        bits = q.cover(n_bytes)
    return lookups, fronts, fin, bits


def time_bed(q, text, n: int, bits, n_bases: int, n_covered: int, runs: int) -> dict:
    """The soft apply with the intervals off and on, 1 warm-up + `runs` runs each; the intervals checked against the counts."""
    res = {}
    for name, on in (("intervals_off", False), ("intervals_on", True)):
        masks, ivs = [], []
        for i in range(runs + 1):
            q.reset()
            q.set_mask(bits, n_bases)
            if on:
                q.set_intervals(True)
            q.feed_device(text.ptr, n)
            done = q.finish()
            if i:
                masks.append(float(q.timings()["mask_s"]))
                if on:
                    ivs.append(q.interval_seconds())
        masked, seen = q.mask_counts(done["n_records"])
        assert seen == n_bases and int(masked.sum()) == n_covered, "the masked bases are not the covered ones"
        res[name] = {"mask_s_runs": masks, "mask_s_median": statistics.median(masks)}
        if on:
            rec, start, end = q.intervals()
            assert int((end - start).sum()) == n_covered and bool((rec[1:] >= rec[:-1]).all()), "the intervals do not add up to the masked bases"
            res[name].update(intervals_s_runs=ivs, intervals_s_median=statistics.median(ivs), n_intervals=int(rec.size),
                             mean_interval_bp=n_covered / max(1, int(rec.size)))
    return res


def main():
    argv, args, runs, bed = sys.argv[1:], [], 5, False
    while argv:
        a = argv.pop(0)
        if a == "--runs":
            runs = int(argv.pop(0))
        elif a == "--bed":
            bed = True
        elif not a.startswith("--"):
            args.append(a)
    genome_bp = int(os.environ.get("PK_QUERY_BENCH_BP", 800_000_000))
    table_bp = int(os.environ.get("PK_QUERY_BENCH_TABLE_BP", 40_000_000))
    if _lib.device_count() < 1:
        sys.exit("error: mask_bench.py needs a GPU")
    bufs = query_bench.stage_tables(table_bp)
    ptrs = [b.ptr for b in bufs]
    hip = filter_bench.hip_runtime()
    out = {"k": K, "n_tables": query_bench.N, "table_genome_bp": table_bp, "runs": runs,
           "method": f"per configuration 1 warm-up + median of {runs} runs; lookup_s and mask_s from HIP events (pk_indexer_timings) around the kernels "
                     "behind the squeeze; copy_s: hipMemcpyDtoDAsync of the same text between two HIP events, same process"}
    if bed:
        out["method"] = (f"per configuration 1 warm-up + median of {runs} runs, both configurations in one process; mask_s from HIP events around "
                         "k_mask_apply (pk_indexer_timings), intervals_s from the HIP events of the interval kernels (pk_query_interval_count); copy_s: "
                         "hipMemcpyDtoDAsync of the same text between two HIP events")
        out["text_reads"] = ("k_iv_count stages every chunk of the text once; k_iv_write stages the chunks that hold a start or an end once more; "
                             "k_coords_sum stages the chunks that hold a piece that is not plain sequence text")
    for name, make in query_bench.shapes(genome_bp):
        fa, bp = make()
        n = len(fa)
        text, scratch = _lib.DeviceBuffer(n + 64), _lib.DeviceBuffer(n + 64)
        text.upload(np.asarray(fa))
        del fa
        if bed:
            with _lib.QueryIndexer(K) as q:
                _, _, fin, (bits, n_bases) = time_lookup(q, text, n, ptrs, 0, True)
            n_covered = count_bits(bits, n_bases)
            res = out[name] = {"bp": int(bp), "text_bytes": n, "records": fin["n_records"], "n_bases": n_bases, "covered_bases": n_covered}
            with _lib.QueryIndexer(1) as q:
                res.update(time_bed(q, text, n, bits, n_bases, n_covered, runs))
            copies = filter_bench.time_copy(hip, scratch.ptr, text.ptr, n, runs)
            copy, apply_s, iv_s = statistics.median(copies), res["intervals_off"]["mask_s_median"], res["intervals_on"]["intervals_s_median"]
            res.update(copy_s_runs=copies, copy_s_median=copy, copy_GB_per_s=n / copy / 1e9, intervals_over_apply=iv_s / apply_s,
                       intervals_over_copy=iv_s / copy, apply_on_over_off=res["intervals_on"]["mask_s_median"] / apply_s,
                       intervals_text_GB_per_s=n / iv_s / 1e9)
            print(name, json.dumps(res), flush=True)
            text.free()
            scratch.free()
            continue
        with _lib.QueryIndexer(K) as q:
            plain, front, fin, _ = time_lookup(q, text, n, ptrs, runs, False)
            covered, _, _, (bits, n_bases) = time_lookup(q, text, n, ptrs, runs, True)
        n_covered = count_bits(bits, n_bases)
        res = out[name] = {"bp": int(bp), "text_bytes": n, "records": fin["n_records"], "windows": fin["num_kmers"], "n_bases": n_bases,
                           "covered_bases": n_covered, "plain_lookup_s_runs": plain, "plain_lookup_s_median": statistics.median(plain),
                           "cover_lookup_s_runs": covered, "cover_lookup_s_median": statistics.median(covered),
                           "cover_over_plain_lookup": statistics.median(covered) / statistics.median(plain),
                           "structure_plus_squeeze_s_median": statistics.median(front), "apply": {}}
        with _lib.QueryIndexer(1) as q:
            for mode, hard in (("soft", False), ("hard", True)):
                times = []
                for i in range(runs + 1):
                    q.reset()
                    q.set_mask(bits, n_bases, hard=hard)
                    q.feed_device(text.ptr, n)
                    done = q.finish()
                    if i:
                        times.append(float(q.timings()["mask_s"]))
                masked, seen = q.mask_counts(done["n_records"])
                assert seen == n_bases and int(masked.sum()) == n_covered, "the masked bases are not the covered ones"
                med = statistics.median(times)
                res["apply"][mode] = {"mask_s_runs": times, "mask_s_median": med, "text_GB_per_s": n / med / 1e9}
        copies = filter_bench.time_copy(hip, scratch.ptr, text.ptr, n, runs)
        copy = statistics.median(copies)
        res.update(copy_s_runs=copies, copy_s_median=copy, copy_GB_per_s=n / copy / 1e9,
                   apply_over_copy={m: v["mask_s_median"] / copy for m, v in res["apply"].items()})
        print(name, json.dumps(res), flush=True)
        text.free()
        scratch.free()
    for b in bufs:
        b.free()
    path = args[0] if args else os.path.join(ROOT, "profiles", "mask_bed_k15_n13.json" if bed else "mask_k15_n13.json")
    with open(path + ".tmp", "w") as fh:
        json.dump(out, fh, indent=1)
    os.replace(path + ".tmp", path)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
