"""Times the FASTQ front end (fastq.hip) against the FASTA pipeline behind it, at k = 15.

The read set: 150 bp reads with 1 % substitutions and 0.2 % N, sampled from either strand of a synthetic genome
(synth.generate), about 1 Gbp (PK_BENCH_FASTQ_BP to change it); quality bytes uniform in 33 .. 73.  The FASTQ and its FASTA
equivalent (what tests/fastq_ref.fastq_to_fasta makes of it) are uploaded to HBM once and fed through
pk_indexer_feed_device: one warm-up, then the median of 5 timed runs (reset, feed, finish) each.

    python tools/bench_fastq.py [out.json]             wall times; with a rocprofv3 kernel-trace run of its own (a child
                                                      process: `rocprofv3 --kernel-trace --stats ... -- python
                                                      tools/bench_fastq.py --once`), the front end's share of device time
    python tools/bench_fastq.py --once                 one FASTQ and one FASTA pass (what the profiled child runs)
    --min-qual Q                                       the FASTQ passes mask the bases below quality Q (offset 33; README "Base
                                                      quality"): k_fq_mask joins the front end, and the FASTA passes count
                                                      other text (the unmasked one), so the two are no longer compared
    --reads FILE.npz                                   keep the read set in FILE (made on the first use): the ~1 Gbp set takes
                                                      longer to build than every pass on it together

Writes profiles/fastq_1gbp.json (fastq_qual_1gbp_q<Q>.json with --min-qual; or out.json) and, next to it, the kernel stats
as <name>_kernel_stats.csv."""
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import fastq_ref  # noqa: E402
import synth  # noqa: E402
from pykmer_amd import _lib  # noqa: E402

K = 15
READ_LEN = 150
FRONT_END = ("k_fq_count", "k_fq_scan", "k_fq_write", "k_fq_check", "k_fq_mask")
QUAL_OFFSET = 33
QUAL_LO, QUAL_HI = 33, 74                                                   # fastq_ref.read_set draws the quality bytes from [33, 74)


def read_set(total_bp: int, cache: str = None):
    if cache and os.path.exists(cache):
        z = np.load(cache)
        if int(z["total_bp"]) == total_bp:
            return z["fq"].tobytes(), z["fa"].tobytes()
    fa_genome, _ = synth.generate(7, 60_000_000, 8, pm_dup=100, pm_tandem=50, pm_ngap=10, pm_lower=20)
    text = np.asarray(fa_genome)
    keep = np.isin(text, np.frombuffer(b"ACGTacgt", dtype=np.uint8))      # the bases of all records back to back
    bases = text[keep] & 0xDF
    codes = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), bases).astype(np.uint8)
    fq, fa = fastq_ref.read_set(total_bp // READ_LEN, length=READ_LEN, seed=1, genome=codes)
    if cache:
        with open(cache + ".tmp", "wb") as fh:
            np.savez(fh, fq=np.frombuffer(fq, dtype=np.uint8), fa=np.frombuffer(fa, dtype=np.uint8), total_bp=np.int64(total_bp))
        os.replace(cache + ".tmp", cache)
    return fq, fa


def once(fq_dev, fq_n, fa_dev, fa_n, min_qual: int = 0):
    """One reset + feed + finish per format; seconds each."""
    out = {}
    for fmt, ptr, n in (("fastq", fq_dev, fq_n), ("fasta", fa_dev, fa_n)):
        extra = {"min_qual_byte": min_qual + QUAL_OFFSET} if fmt == "fastq" and min_qual else {}
        with _lib.Indexer(K, fmt=fmt, **extra) as ix:
            ix.feed_device(ptr, n)                                         # warm-up: allocations
            ix.finish()
            times = []
            for _ in range(5):
                ix.reset()
                t0 = time.perf_counter()
                ix.feed_device(ptr, n)
                fin = ix.finish()
                times.append(time.perf_counter() - t0)
            out[fmt] = {"median_s": statistics.median(times), "best_s": min(times), "worst_s": max(times), "num_kmers": fin["num_kmers"],
                        "n_records": fin["n_records"], "timings": ix.timings()}
            if fmt == "fastq":
                out[fmt]["stats"] = ix.fastq_stats()
                if min_qual:
                    out[fmt]["masked"] = ix.fastq_masked()
    return out


def kernel_stats(argv, keep_as: str):
    """Runs `argv` under rocprofv3 --kernel-trace --stats; returns the rows of its kernel stats CSV (copied to `keep_as`)."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    d = tempfile.mkdtemp(prefix="fqprof")
    subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "fq", "--"] + argv,
                   check=True, timeout=1800, cwd=ROOT)
    path = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
    with open(path) as fh:
        rows = list(csv.DictReader(fh))
    shutil.copy(path, keep_as)
    shutil.rmtree(d, ignore_errors=True)
    return rows


def launches(rows) -> dict:
    """Kernel name (without namespaces, template and call arguments) -> launches, over the library's kernels."""
    out = {}
    for r in rows:
        if "pk::" in r["Name"]:
            name = re.sub(r"\(anonymous namespace\)::", "", r["Name"]).split("(")[0].split("<")[0].split("::")[-1]
            out[name] = out.get(name, 0) + int(r["Calls"])
    return out


def _option(name: str):
    """The value behind `name` in sys.argv, or None."""
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None


def main():
    min_qual = int(_option("--min-qual") or 0)
    cache = _option("--reads")
    values = {v for v in (_option("--min-qual"), cache) if v is not None}
    args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in values]
    if not 0 <= min_qual <= 255 - QUAL_OFFSET:
        sys.exit(f"error: --min-qual must lie in 0..{255 - QUAL_OFFSET}")
    total_bp = int(os.environ.get("PK_BENCH_FASTQ_BP", 1_000_000_000))
    fq, fa = read_set(total_bp, cache)
    bufs = []
    for data in (fq, fa):
        b = _lib.DeviceBuffer(len(data))
        b.upload(np.frombuffer(data, dtype=np.uint8))
        bufs.append(b)
    res = once(bufs[0].ptr, len(fq), bufs[1].ptr, len(fa), min_qual)
    if "--once" in sys.argv:
        return
    for b in bufs:
        b.free()
    default = f"fastq_qual_1gbp_q{min_qual}.json" if min_qual else "fastq_1gbp.json"
    path = args[0] if args else os.path.join(ROOT, "profiles", default)
    out = {"k": K, "read_len": READ_LEN, "reads": res["fastq"]["n_records"], "fastq_bytes": len(fq), "fasta_bytes": len(fa),
           "bp": res["fastq"]["n_records"] * READ_LEN, "wall": res,
           "wall_ratio_fastq_over_fasta": round(res["fastq"]["median_s"] / res["fasta"]["median_s"], 3)}
    if min_qual:
        bp = out["bp"]
        out["min_qual"] = {"Q": min_qual, "offset": QUAL_OFFSET, "masked": res["fastq"]["masked"], "share_masked": round(res["fastq"]["masked"] / bp, 4),
                           "share_expected": round((min_qual + QUAL_OFFSET - QUAL_LO) / (QUAL_HI - QUAL_LO), 4)}
    else:
        out["same_counts"] = res["fastq"]["num_kmers"] == res["fasta"]["num_kmers"]
    child = [sys.executable, os.path.abspath(__file__), "--once"] + (["--min-qual", str(min_qual)] if min_qual else []) + (["--reads", cache] if cache else [])
    rows = kernel_stats(child, os.path.splitext(path)[0] + "_kernel_stats.csv")
    runs = 12                                                              # two indexers x (warm-up + 5) feeds, fed once each
    front = sum(int(r["TotalDurationNs"]) for r in rows if any(f in r["Name"] for f in FRONT_END))
    pk = sum(int(r["TotalDurationNs"]) for r in rows if "pk::" in r["Name"])
    fasta_pipeline_per_run = (pk - front) / runs                           # text of the same size runs through it for both formats
    front_per_run = front / (runs / 2)
    moved = len(fq) + res["fastq"]["stats"]["bytes_emitted"]               # read once, written once (the count pass reads again)
    reads_of_feed = 3 if min_qual else 2                                   # k_fq_count, k_fq_write and, masking, k_fq_mask each read the feed
    out["device"] = {
        "front_end_ms_per_feed": round(front_per_run / 1e6, 3),
        "front_end_by_kernel_ms": {f: round(sum(int(r["TotalDurationNs"]) for r in rows if f in r["Name"]) / (runs / 2) / 1e6, 3)
                                   for f in FRONT_END},
        "launches": launches(rows),
        "fasta_pipeline_ms_per_feed": round(fasta_pipeline_per_run / 1e6, 3),
        "front_end_share_of_fasta_pipeline": round(front_per_run / fasta_pipeline_per_run, 3),
        "front_end_gb_per_s_in_plus_out": round(moved / front_per_run, 1),
        "front_end_gb_per_s_min_traffic": round((reads_of_feed * len(fq) + res["fastq"]["stats"]["bytes_emitted"]) / front_per_run, 1),
        "target_share": 0.15,
    }
    if not min_qual:
        out["device"]["target_met"] = out["device"]["front_end_share_of_fasta_pipeline"] <= 0.15
    with open(path + ".tmp", "w") as fh:
        json.dump(out, fh, indent=1)
    os.replace(path + ".tmp", path)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
