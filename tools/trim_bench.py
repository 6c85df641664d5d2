"""Times the three device phases of trim.py on the read set of tools/query_bench.py turned into FASTQ: 400 000 reads of 1 kbp
(synth.generate(34, 400_000_000, 400_000), every record's sequence on one line, qualities drawn like fastq_ref.read_set's),
k = 15, N = 13 tables counted from synth.family, text and tables in HBM.  With `--reads cache.npz` (the cache file of
tools/bench_fastq.py) the 150 bp read set of that tool is timed as a second shape.

Per shape, in one process: the cover lookup of phase 1 (pk_query_set_cover on FASTQ input: `lookup_s` of pk_indexer_timings,
HIP events around k_cover_scan + k_query_cover; the FASTQ front end, the structure pass and the squeeze are reported beside
it, not in it), the trim kernels of phase 2 (pk_trim_feed_device of the whole text: `trim_s` of pk_trim_timings, HIP events
around k_trim_count + k_trim_scan + k_trim_runs), the select kernels of phase 3 (pk_select_feed_device over the nine segments
per read of trim.trim_segments: `select_s` of pk_select_timings), and hipMemcpyDtoDAsync of the same text between two HIP
events on the null stream, as tools/filter_bench.py times it.  Per phase one warm-up, then the median of `--runs` timed runs
(5), each with a fresh object.  Once per shape the trimmer's covered bases are checked against the set bits of phase 1.

    python tools/trim_bench.py [out.json] [--runs R] [--min-len L] [--reads cache.npz]
    PK_QUERY_BENCH_BP / PK_QUERY_BENCH_TABLE_BP scale the read set and the table genomes down for a rehearsal.

Writes profiles/trim_k15_n13.json (or out.json)."""
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
from pykmer_amd import _lib, trim  # noqa: E402
from pykmer_amd.mask import count_bits  # noqa: E402

K = query_bench.K


def fastq_of(fa, seed: int = 1):
    """(fastq bytes, record offsets (R + 1,) uint64) of a FASTA text: every record's lines joined into line 2, a '+' line and
    qualities from [33, 74)."""
    pool = np.random.default_rng(seed).integers(33, 74, 1 << 22, dtype=np.uint8).tobytes()
    out, starts, pos, at = [], [], 0, 0
    for rec in bytes(fa).split(b">")[1:]:
        name, _, body = rec.partition(b"\n")
        seq = body.replace(b"\n", b"")
        if at + len(seq) > len(pool):
            at = 0
        rec = b"@" + name + b"\n" + seq + b"\n+\n" + pool[at:at + len(seq)] + b"\n"
        at += 61
        starts.append(pos)
        pos += len(rec)
        out.append(rec)
    return b"".join(out), np.array(starts + [pos], dtype=np.uint64)


def record_starts_of(fq: bytes) -> np.ndarray:
    """The record offsets of a FASTQ text whose every line ends with one \\n and whose records are four lines."""
    a = np.frombuffer(fq, dtype=np.uint8)
    nl = np.flatnonzero(a == 10)
    assert nl.size % 4 == 0 and nl.size and int(nl[-1]) == a.size - 1
    return np.concatenate([[0], nl[3::4] + 1]).astype(np.uint64)


def time_shape(name: str, fq: bytes, starts: np.ndarray, ptrs, hip, runs: int, min_len: int) -> dict:
    n, R = len(fq), starts.size - 1
    text, scratch = _lib.DeviceBuffer(n + 64), _lib.DeviceBuffer(n + 64)
    text.upload(np.frombuffer(fq, dtype=np.uint8))
    try:
        lookups, fronts = [], []
        with _lib.QueryIndexer(K, fmt="fastq") as q:
            for i in range(runs + 1):
                q.reset()
                q.set_tables(ptrs, 1, 255)
                q.set_cover(True)
                q.feed_device(text.ptr, n)
                fin = q.finish()
                if i:
                    t = q.timings()
                    lookups.append(float(t["lookup_s"]))
                    fronts.append(float(t["scan_s"] + t["squeeze_s"]))
            bits, n_bases = q.cover(n)
            bits = bits.copy()
        assert fin["n_records"] == R
        n_covered = count_bits(bits, n_bases)
        print(name, "lookup", lookups, flush=True)
        trims = []
        for i in range(runs + 1):
            with _lib.Trimmer(0) as t:
                t.set_cover(bits, n_bases)
                got = t.feed_device(text.ptr, n, starts)
                done = t.finish()
                if i:
                    trims.append(t.timings()["trim_s"])
        assert done == {"n_records": R, "n_bases": n_bases, "n_covered": n_covered}, "the trimmer's covered bases are not the set bits"
        print(name, "trim", trims, flush=True)
        keep = trim.decide(got["trim_start"], got["trim_end"], min_len)
        offsets, flags = trim.trim_segments(starts, got, got["trim_start"], got["trim_end"], keep)
        selects = []
        for i in range(runs + 1):
            with _lib.Selector(0) as sel:
                sel.set_records(offsets, flags)
                kept = sel.feed_device(text.ptr, n, scratch.ptr, n)
                if i:
                    selects.append(sel.timings()["select_s"])
        print(name, "select", selects, flush=True)
        copies = filter_bench.time_copy(hip, scratch.ptr, text.ptr, n, runs)
        length = (got["trim_end"] - got["trim_start"]).astype(np.int64)
        lookup, trim_s, select, copy = (statistics.median(v) for v in (lookups, trims, selects, copies))
        return {"text_bytes": n, "records": R, "bp": int(got["seq_len"].sum()), "n_bases": n_bases, "covered_bases": n_covered, "min_len": min_len,
                "reads_kept": int(keep.sum()), "reads_whole": int(((keep != 0) & (length == got["seq_len"].astype(np.int64))).sum()),
                "bases_kept": int(length[keep != 0].sum()), "bytes_kept": int(kept),
                "cover_lookup_s_runs": lookups, "cover_lookup_s_median": lookup, "structure_plus_squeeze_s_median": statistics.median(fronts),
                "trim_s_runs": trims, "trim_s_median": trim_s, "select_s_runs": selects, "select_s_median": select,
                "copy_s_runs": copies, "copy_s_median": copy, "copy_GB_per_s": n / copy / 1e9, "trim_text_GB_per_s": n / trim_s / 1e9,
                "trim_over_copy": trim_s / copy, "trim_over_cover_lookup": trim_s / lookup, "select_over_copy": select / copy}
    finally:
        text.free()
        scratch.free()


def main():
    argv, args, runs, min_len, cache = sys.argv[1:], [], 5, 100, None
    while argv:
        a = argv.pop(0)
        if a == "--runs":
            runs = int(argv.pop(0))
        elif a == "--min-len":
            min_len = int(argv.pop(0))
        elif a == "--reads":
            cache = argv.pop(0)
        elif not a.startswith("--"):
            args.append(a)
    genome_bp = int(os.environ.get("PK_QUERY_BENCH_BP", 800_000_000))
    table_bp = int(os.environ.get("PK_QUERY_BENCH_TABLE_BP", 40_000_000))
    if _lib.device_count() < 1:
        sys.exit("error: trim_bench.py needs a GPU")
    bufs = query_bench.stage_tables(table_bp)
    ptrs = [b.ptr for b in bufs]
    print("tables staged", flush=True)
    hip = filter_bench.hip_runtime()
    out = {"k": K, "n_tables": query_bench.N, "table_genome_bp": table_bp, "runs": runs,
           "method": f"per phase 1 warm-up + median of {runs} runs with a fresh object each, one process; cover_lookup_s from HIP events around "
                     "k_cover_scan + k_query_cover (pk_indexer_timings, FASTQ input), trim_s around k_trim_count + k_trim_scan + k_trim_runs "
                     "(pk_trim_timings), select_s around the select kernels over nine segments per read (pk_select_timings); copy_s: "
                     "hipMemcpyDtoDAsync of the same text between two HIP events",
           "text_reads": "k_trim_count reads lines 1-3 of every record once and line 2 a second time; k_trim_runs reads line 2 once more and the "
                         "cover bits once; line 4 is read only with a quality threshold"}
    fa, _ = synth.generate(34, genome_bp // 2, max(1, genome_bp // 2000))
    fq, starts = fastq_of(fa)
    del fa
    print("reads made", len(fq), flush=True)
    out["reads_1kbp"] = time_shape("reads_1kbp", fq, starts, ptrs, hip, runs, min_len)
    print("reads_1kbp", json.dumps(out["reads_1kbp"]), flush=True)
    del fq
    if cache and os.path.exists(cache):
        fq = np.load(cache)["fq"].tobytes()
        out["reads_150bp"] = time_shape("reads_150bp", fq, record_starts_of(fq), ptrs, hip, runs, min(min_len, 50))
        print("reads_150bp", json.dumps(out["reads_150bp"]), flush=True)
    for b in bufs:
        b.free()
    path = args[0] if args else os.path.join(ROOT, "profiles", "trim_k15_n13.json")
    with open(path + ".tmp", "w") as fh:
        json.dump(out, fh, indent=1)
    os.replace(path + ".tmp", path)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
