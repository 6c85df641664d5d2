"""Times the correct kernels of correct.py on the read set of tools/query_bench.py turned into FASTQ (tools/trim_bench.py's):
400 000 reads of 1 kbp, k = 15, N = 13 tables counted from synth.family, text and tables in HBM.

In one process: the cover lookup of the first pass (pk_query_set_cover on FASTQ input: `lookup_s` of pk_indexer_timings), the
correct kernels of the second (pk_correct_feed_device of the whole text: `correct_s` of pk_correct_timings, HIP events around
k_trim_count + k_trim_scan + k_correct_runs; the copy of the text that the kernels patch is outside them), and
hipMemcpyDtoDAsync of the same text between two HIP events on the null stream, as tools/filter_bench.py times it.  Per phase
one warm-up, then the median of `--runs` timed runs (5), each with a fresh object.  The candidates and the tried candidates
(candidates - untried) are reported, and the time per tried candidate.  Not measured: end-to-end wall time, and a run with a
quality threshold.

    python tools/correct_bench.py [out.json] [--runs R] [--min-windows M]
    PK_QUERY_BENCH_BP / PK_QUERY_BENCH_TABLE_BP scale the read set and the table genomes down for a rehearsal.

Writes profiles/correct_k15_n13.json (or out.json)."""
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
import synth  # noqa: E402
import trim_bench  # noqa: E402
from pykmer_amd import _lib  # noqa: E402
from pykmer_amd.correct import validate_min_windows  # noqa: E402

K = query_bench.K


def time_shape(name: str, fq: bytes, starts: np.ndarray, ptrs, hip, runs: int, min_windows: int) -> dict:
    n, R = len(fq), starts.size - 1
    text, patched = _lib.DeviceBuffer(n + 64), _lib.DeviceBuffer(n + 64)
    text.upload(np.frombuffer(fq, dtype=np.uint8))
    try:
        lookups = []
        with _lib.QueryIndexer(K, fmt="fastq") as q:
            for i in range(runs + 1):
                q.reset()
                q.set_tables(ptrs, 1, 255)
                q.set_cover(True)
                q.feed_device(text.ptr, n)
                fin = q.finish()
                if i:
                    lookups.append(float(q.timings()["lookup_s"]))
            bits, n_bases = q.cover(n)
            bits = bits.copy()
        assert fin["n_records"] == R
        print(name, "lookup", lookups, flush=True)
        corrects = []
        for i in range(runs + 1):
            with _lib.Corrector(K, 0) as c:
                c.set_tables(ptrs, 1, 255)
                c.set_cover(bits, n_bases, 0, min_windows)
                got = c.feed_device(text.ptr, n, starts, patched.ptr)
                done = c.finish()
                if i:
                    corrects.append(c.timings()["correct_s"])
        assert done["n_records"] == R and done["n_bases"] == n_bases
        print(name, "correct", corrects, flush=True)
        changed = int((patched.download()[:n] != np.frombuffer(fq, dtype=np.uint8)).sum())
        assert changed == done["n_corrected"], "the bytes that differ are not the corrected positions"
        copies = filter_bench.time_copy(hip, patched.ptr, text.ptr, n, runs)
        lookup, correct_s, copy = (statistics.median(v) for v in (lookups, corrects, copies))
        tried = done["n_candidates"] - done["n_untried"]
        return {"text_bytes": n, "records": R, "bp": int(got["seq_len"].sum()), "n_bases": n_bases, "min_windows": min_windows,
                "candidates": done["n_candidates"], "untried": done["n_untried"], "tried": tried, "corrected": done["n_corrected"],
                "ambiguous": done["n_ambiguous"], "unfixable": tried - done["n_corrected"] - done["n_ambiguous"],
                "reads_with_a_candidate": int((got["candidates"] > 0).sum()),
                "cover_lookup_s_runs": lookups, "cover_lookup_s_median": lookup, "correct_s_runs": corrects, "correct_s_median": correct_s,
                "copy_s_runs": copies, "copy_s_median": copy, "copy_GB_per_s": n / copy / 1e9, "correct_text_GB_per_s": n / correct_s / 1e9,
                "correct_over_copy": correct_s / copy, "correct_over_cover_lookup": correct_s / lookup,
                "correct_ns_per_tried_candidate": correct_s / max(1, tried) * 1e9}
    finally:
        text.free()
        patched.free()


def main():
    argv, args, runs, min_windows = sys.argv[1:], [], 5, None
    while argv:
        a = argv.pop(0)
        if a == "--runs":
            runs = int(argv.pop(0))
        elif a == "--min-windows":
            min_windows = int(argv.pop(0))
        elif not a.startswith("--"):
            args.append(a)
    min_windows = validate_min_windows(min_windows, K)
    genome_bp = int(os.environ.get("PK_QUERY_BENCH_BP", 800_000_000))
    table_bp = int(os.environ.get("PK_QUERY_BENCH_TABLE_BP", 40_000_000))
    if _lib.device_count() < 1:
        sys.exit("error: correct_bench.py needs a GPU")
    bufs = query_bench.stage_tables(table_bp)
    ptrs = [b.ptr for b in bufs]
    print("tables staged", flush=True)
    hip = filter_bench.hip_runtime()
    out = {"k": K, "n_tables": query_bench.N, "table_genome_bp": table_bp, "runs": runs,
           "method": f"per phase 1 warm-up + median of {runs} runs with a fresh object each, one process; cover_lookup_s from HIP events around "
                     "k_cover_scan + k_query_cover (pk_indexer_timings, FASTQ input), correct_s around k_trim_count + k_trim_scan + k_correct_runs "
                     "(pk_correct_timings; the copy of the text that is patched is outside them); copy_s: hipMemcpyDtoDAsync of the same text "
                     "between two HIP events",
           "not_measured": "end-to-end wall time of correct.py; a run with a quality threshold"}
    fa, _ = synth.generate(34, genome_bp // 2, max(1, genome_bp // 2000))
    fq, starts = trim_bench.fastq_of(fa)
    del fa
    print("reads made", len(fq), flush=True)
    out["reads_1kbp"] = time_shape("reads_1kbp", fq, starts, ptrs, hip, runs, min_windows)
    for b in bufs:
        b.free()
    path = args[0] if args else os.path.join(ROOT, "profiles", "correct_k15_n13.json")
    with open(path + ".tmp", "w") as fh:
        json.dump(out, fh, indent=1)
    os.replace(path + ".tmp", path)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
