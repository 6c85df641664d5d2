"""Times k_patterns (pk_patterns_device_accumulate) on tables of 4^15 bytes resident in HBM, each time set against ONE
single-window scan (pk_gram_device_partial) and one occgram pass (pk_occgram_device_accumulate) of the same tables in the
same process.  Kernel seconds from HIP events: median (and best) of 5 after 1 warm-up.  Table sets:
  genome        synth.family(i, 40_000_000) counted by the indexer (the bench's merge set), N = 13
  dense_genome  synth.family(i, 400_000_000), N = 13
  genome_n16    the genome set at N = 16 (four launches over the tables)
  identical     13 copies of one genome table: every held address falls into one bin
Before timing, matrix_from_patterns of the pass must equal the scan's pair tallies and the patterns must sum to 4^15; at
window 1-255 the occupancy classes must equal the occgram pass's occ_hist.  A pass at window 2-255 (the general window
test) is timed beside the 1-255 one.  Writes one JSON line per set to stdout and all of them to
profiles/patterns_k15.json (or the path given as the first argument; a second argument picks sets by name)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_spectrum import genome_tables, n  # noqa: E402
from pykmer_amd import _lib, kwip, patterns  # noqa: E402


def run_patterns(ptrs, acc, window=(1, 255)):
    acc.zero_()
    torch.cuda.synchronize()
    return _lib.patterns_device_accumulate(ptrs, n, acc.data_ptr(), *window)


def measure(name, tabs):
    N = len(tabs)
    ptrs = [t.data_ptr() for t in tabs]
    acc = torch.zeros(_lib.patterns_words(N), dtype=torch.int64, device="cuda")
    occ = torch.zeros(_lib.occgram_words(N), dtype=torch.int64, device="cuda")
    run_patterns(ptrs, acc)
    bins = acc.cpu().numpy().view(np.uint64).copy()
    pair, _ = _lib.gram_device_partial(ptrs, n)
    assert int(bins.sum()) == n, "the patterns do not sum to the table size"
    assert np.array_equal(patterns.matrix_from_patterns(bins, N), pair), "the patterns disagree with the scan's pair tallies"
    pat_t, gen_t, scan_t, occ_t = [], [], [], []
    for rep in range(6):
        p = run_patterns(ptrs, acc)
        g = run_patterns(ptrs, acc, (2, 255))
        _, s = _lib.gram_device_partial(ptrs, n)
        occ.zero_()
        torch.cuda.synchronize()
        o = _lib.occgram_device_accumulate(ptrs, n, occ.data_ptr())
        if rep:
            pat_t.append(p)
            gen_t.append(g)
            scan_t.append(s)
            occ_t.append(o)
    occ_hist = kwip.split_accumulator(occ.cpu().numpy().view(np.uint64), N)[0]
    assert np.array_equal(patterns.occupancy_from_patterns(bins, N), occ_hist), "the patterns disagree with the occgram pass's occ_hist"
    held = n - int(bins[0])
    ms = lambda ts: round(statistics.median(ts) * 1e3, 3)                    # noqa: E731
    out = {"set": name, "N": N, "table_bytes": n, "held_fraction": round(held / n, 4), "n_patterns": int(np.count_nonzero(bins[1:])),
           "hottest_bin_share": round(int(bins[1:].max()) / max(1, held), 4), "launches": 1 << max(0, N - 14),
           "patterns_ms_median": ms(pat_t), "patterns_ms_best": round(min(pat_t) * 1e3, 3), "patterns_2_255_ms_median": ms(gen_t),
           "scan_ms_median": ms(scan_t), "scan_ms_best": round(min(scan_t) * 1e3, 3), "occgram_ms_median": ms(occ_t),
           "ratio_to_scan": round(statistics.median(pat_t) / statistics.median(scan_t), 2),
           "ratio_to_occgram": round(statistics.median(pat_t) / statistics.median(occ_t), 3),
           "read_tb_per_s": round(N * n * (1 << max(0, N - 14)) / statistics.median(pat_t) / 1e12, 2), "exact": True}
    print(json.dumps(out), flush=True)
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "patterns_k15.json")
    only = set(sys.argv[2].split(",")) if len(sys.argv) > 2 else None
    want = lambda name: not only or name in only                              # noqa: E731
    results = []
    if want("genome") or want("genome_n16") or want("identical"):
        tabs = genome_tables(16 if want("genome_n16") else 13, 40_000_000)
        if want("genome"):
            results.append(measure("genome", tabs[:13]))
        if want("genome_n16"):
            results.append(measure("genome_n16", tabs))
        if want("identical"):
            del tabs[1:]
            torch.cuda.empty_cache()
            results.append(measure("identical", tabs + [tabs[0].clone() for _ in range(12)]))
        del tabs
        torch.cuda.empty_cache()
    if want("dense_genome"):
        tabs = genome_tables(13, 400_000_000)
        results.append(measure("dense_genome", tabs))
        del tabs
        torch.cuda.empty_cache()
    with open(path + ".tmp", "w") as fh:
        json.dump({"kernel": "k_patterns", "device": torch.cuda.get_device_name(0), "results": results}, fh, indent=1)
    os.replace(path + ".tmp", path)


if __name__ == "__main__":
    main()
