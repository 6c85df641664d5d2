"""Times the FASTQ front end (fastq.hip) against the FASTA pipeline behind it, at k = 15.

The read set: 150 bp reads with 1 % substitutions and 0.2 % N, sampled from either strand of a synthetic genome
(synth.generate), about 1 Gbp (PK_BENCH_FASTQ_BP to change it).  The FASTQ and its FASTA equivalent (what
tests/fastq_ref.fastq_to_fasta makes of it) are uploaded to HBM once and fed through pk_indexer_feed_device: one warm-up,
then the median of 5 timed runs (reset, feed, finish) each.

    python tools/bench_fastq.py [out.json]             wall times; with a rocprofv3 kernel-trace run of its own (a child
                                                      process: `rocprofv3 --kernel-trace --stats ... -- python
                                                      tools/bench_fastq.py --once`), the front end's share of device time
    python tools/bench_fastq.py --once                 one FASTQ and one FASTA pass (what the profiled child runs)

Writes profiles/fastq_1gbp.json (or out.json) and profiles/fastq_1gbp_kernel_stats.csv."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import fastq_ref  # noqa: E402
import synth  # noqa: E402
from pykmer_amd import _lib  # noqa: E402

K = 15
READ_LEN = 150
FRONT_END = ("k_fq_count", "k_fq_scan", "k_fq_write", "k_fq_check")


def read_set(total_bp: int):
    fa_genome, _ = synth.generate(7, 60_000_000, 8, pm_dup=100, pm_tandem=50, pm_ngap=10, pm_lower=20)
    text = np.asarray(fa_genome)
    keep = np.isin(text, np.frombuffer(b"ACGTacgt", dtype=np.uint8))      # the bases of all records back to back
    bases = text[keep] & 0xDF
    codes = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), bases).astype(np.uint8)
    return fastq_ref.read_set(total_bp // READ_LEN, length=READ_LEN, seed=1, genome=codes)


def once(fq_dev, fq_n, fa_dev, fa_n):
    """One reset + feed + finish per format; seconds each."""
    out = {}
    for fmt, ptr, n in (("fastq", fq_dev, fq_n), ("fasta", fa_dev, fa_n)):
        with _lib.Indexer(K, fmt=fmt) as ix:
            ix.feed_device(ptr, n)                                         # warm-up: allocations
            ix.finish()
            times = []
            for _ in range(5):
                ix.reset()
                t0 = time.perf_counter()
                ix.feed_device(ptr, n)
                fin = ix.finish()
                times.append(time.perf_counter() - t0)
            out[fmt] = {"median_s": statistics.median(times), "best_s": min(times), "num_kmers": fin["num_kmers"],
                        "n_records": fin["n_records"], "timings": ix.timings()}
            if fmt == "fastq":
                out[fmt]["stats"] = ix.fastq_stats()
    return out


def kernel_stats(argv):
    """Runs `argv` under rocprofv3 --kernel-trace --stats; returns the rows of its kernel stats CSV."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    d = tempfile.mkdtemp(prefix="fqprof")
    subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "fq", "--"] + argv,
                   check=True, timeout=1800, cwd=ROOT)
    path = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
    with open(path) as fh:
        rows = list(csv.DictReader(fh))
    shutil.copy(path, os.path.join(ROOT, "profiles", "fastq_1gbp_kernel_stats.csv"))
    shutil.rmtree(d, ignore_errors=True)
    return rows


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    total_bp = int(os.environ.get("PK_BENCH_FASTQ_BP", 1_000_000_000))
    fq, fa = read_set(total_bp)
    bufs = []
    for data in (fq, fa):
        b = _lib.DeviceBuffer(len(data))
        b.upload(np.frombuffer(data, dtype=np.uint8))
        bufs.append(b)
    res = once(bufs[0].ptr, len(fq), bufs[1].ptr, len(fa))
    if "--once" in sys.argv:
        return
    for b in bufs:
        b.free()
    out = {"k": K, "read_len": READ_LEN, "reads": res["fastq"]["n_records"], "fastq_bytes": len(fq), "fasta_bytes": len(fa),
           "bp": res["fastq"]["n_records"] * READ_LEN, "wall": res,
           "wall_ratio_fastq_over_fasta": round(res["fastq"]["median_s"] / res["fasta"]["median_s"], 3),
           "same_counts": res["fastq"]["num_kmers"] == res["fasta"]["num_kmers"]}
    rows = kernel_stats([sys.executable, os.path.abspath(__file__), "--once"])
    runs = 12                                                              # two indexers x (warm-up + 5) feeds, fed once each
    front = sum(int(r["TotalDurationNs"]) for r in rows if any(f in r["Name"] for f in FRONT_END))
    pk = sum(int(r["TotalDurationNs"]) for r in rows if "pk::" in r["Name"])
    fasta_pipeline_per_run = (pk - front) / runs                           # the same text runs through it for both formats
    front_per_run = front / (runs / 2)
    moved = len(fq) + res["fastq"]["stats"]["bytes_emitted"]               # read once, written once (the count pass reads again)
    out["device"] = {
        "front_end_ms_per_feed": round(front_per_run / 1e6, 3),
        "front_end_by_kernel_ms": {f: round(sum(int(r["TotalDurationNs"]) for r in rows if f in r["Name"]) / (runs / 2) / 1e6, 3)
                                   for f in FRONT_END},
        "fasta_pipeline_ms_per_feed": round(fasta_pipeline_per_run / 1e6, 3),
        "front_end_share_of_fasta_pipeline": round(front_per_run / fasta_pipeline_per_run, 3),
        "front_end_gb_per_s_in_plus_out": round(moved / front_per_run, 1),
        "front_end_gb_per_s_min_traffic": round((2 * len(fq) + res["fastq"]["stats"]["bytes_emitted"]) / front_per_run, 1),
        "target_share": 0.15,
    }
    out["device"]["target_met"] = out["device"]["front_end_share_of_fasta_pipeline"] <= 0.15
    path = args[0] if args else os.path.join(ROOT, "profiles", "fastq_1gbp.json")
    with open(path + ".tmp", "w") as fh:
        json.dump(out, fh, indent=1)
    os.replace(path + ".tmp", path)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
