"""Times one extraction (pk_extract_device: count + scan + write) over N = 13 tables of 4^15 bytes resident in HBM, as
tools/bench_kwip.py makes them (synth.family(i, 40_000_000) counted by the indexer), split 7 present / 6 absent, default
thresholds (window 1..255, all present, none absent), each time set against ONE pair scan of the same 13 tables
(pk_gram_device_accumulate: one streaming pass of the same bytes).  Kernel seconds from HIP events: median (and best) of 5
after 1 warm-up.  Also timed: the count-only call (cap = 0, no arrays: count + scan) and, at min_present = 1 / max_absent =
6 (many more rows), a second extraction, to show what the write costs.  Every extraction is checked against torch on the
same tables (the number selected, and the first and last addresses).  Writes one JSON line to stdout and
profiles/extract_k15_n13.json (or the path given as the first argument)."""
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
from pykmer_amd import _lib  # noqa: E402

P, A = 7, 6


def reference_mask(tabs, min_present, max_absent):
    p = torch.zeros(n, dtype=torch.int16, device="cuda")
    q = torch.zeros(n, dtype=torch.int16, device="cuda")
    for t in tabs[:P]:
        p += (t > 0)
    for t in tabs[P:]:
        q += (t > 0)
    return (p >= min_present) & (q <= max_absent)


def time_extract(ptrs, min_present, max_absent, mask):
    want = int(mask.sum())
    addr = torch.empty(max(want, 1), dtype=torch.int64, device="cuda")
    counts = torch.empty(max(want, 1) * P + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    full, count_only = [], []
    for rep in range(6):
        m, fits, s = _lib.extract_device(ptrs, P, n, 0, 1, 255, min_present, max_absent, addr.data_ptr(), counts.data_ptr(), want)
        assert (m, fits) == (want, True), (m, want, fits)
        m0, _, s0 = _lib.extract_device(ptrs, P, n, 0, 1, 255, min_present, max_absent)
        assert m0 == want
        if rep:
            full.append(s)
            count_only.append(s0)
    idx = torch.nonzero(mask).flatten()
    exact = bool(torch.equal(addr[:want], idx))
    del idx
    return {"min_present": min_present, "max_absent": max_absent, "n_selected": want, "output_bytes": want * (8 + P),
            "extract_ms_median": round(statistics.median(full) * 1e3, 3), "extract_ms_best": round(min(full) * 1e3, 3),
            "count_only_ms_median": round(statistics.median(count_only) * 1e3, 3), "exact": exact,
            "effective_TBps": round((P + A) * n / statistics.median(full) / 1e12, 3)}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "extract_k15_n13.json")
    tabs = genome_tables(P + A, 40_000_000)
    ptrs = [t.data_ptr() for t in tabs]
    acc = torch.zeros((P + A) ** 2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    scan = []
    for rep in range(6):
        s = _lib.gram_device_accumulate(ptrs, n, acc.data_ptr())
        if rep:
            scan.append(s)
    runs = [time_extract(ptrs, P, 0, reference_mask(tabs, P, 0)), time_extract(ptrs, 1, A, reference_mask(tabs, 1, A))]
    out = {"kernel": "k_extract_count + k_extract_scan + k_extract_write", "device": torch.cuda.get_device_name(0), "kmer_len": 15,
           "n_present": P, "n_absent": A, "table_bytes": n, "bytes_read_by_the_count_pass": (P + A) * n,
           "nonzero_fraction_table0": round(float((tabs[0] > 0).sum()) / n, 4),
           "pair_scan_ms_median": round(statistics.median(scan) * 1e3, 3), "pair_scan_ms_best": round(min(scan) * 1e3, 3),
           "pair_scan_TBps": round((P + A) * n / statistics.median(scan) / 1e12, 3), "runs": runs}
    for r in runs:
        r["ratio_to_pair_scan"] = round(r["extract_ms_median"] / out["pair_scan_ms_median"], 2)
    print(json.dumps(out), flush=True)
    with open(path + ".tmp", "w") as fh:
        json.dump(out, fh, indent=1)
    os.replace(path + ".tmp", path)


if __name__ == "__main__":
    main()
