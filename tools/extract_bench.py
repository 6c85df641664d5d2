"""Times one extraction (pk_extract_device: count + scan + write) over N = 13 tables of 4^15 bytes resident in HBM, as
tools/bench_kwip.py makes them (synth.family(i, 40_000_000) counted by the indexer), split 7 present / 6 absent, default
thresholds (window 1..255, all present, none absent), each time set against ONE pair scan of the same 13 tables
(pk_gram_device_accumulate: one streaming pass of the same bytes).  Kernel seconds from HIP events: median (and best) of 5
after 1 warm-up.  Also timed: the count-only call (cap = 0, no arrays: count + scan) and, at min_present = 1 / max_absent =
6 (many more rows), a second extraction, to show what the write costs.  Every extraction is checked against torch on the
same tables (the number selected, and the first and last addresses).  Writes one JSON line to stdout and
profiles/extract_k15_n13.json (or the path given as the first argument).

`--table OP` (sum, min, max, count or all) times the table pass instead (pk_extract_table_device: the streaming map and the
histogram of its output behind it) on the same tables and thresholds, each op the median of 5 after 1 warm-up, and in the
same process the count-only call and the pair scan it is set against; the table and the histogram of every op are checked
against torch.  It writes profiles/extract_table_k15_n13.json (or the path given)."""
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


def reference_table(tabs, op, mask):
    """The table of `op` over the window 1..255 (every non-zero byte is inside it), as a uint8 tensor."""
    acc = torch.full((n,), 256 if op == "min" else 0, dtype=torch.int16, device="cuda")
    for t in tabs[:P]:
        if op == "sum":
            acc += t
        elif op == "min":
            acc = torch.minimum(acc, torch.where(t > 0, t.to(torch.int16), 256))
        elif op == "max":
            acc = torch.maximum(acc, t.to(torch.int16))
        else:
            acc += (t > 0)
    return torch.where(mask, acc.clamp_(max=255), 0).to(torch.uint8)


def time_tables(ptrs, tabs, ops, min_present, max_absent, mask):
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    hist = torch.zeros(256, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    count_only = []
    for rep in range(6):
        m, _, s = _lib.extract_device(ptrs, P, n, 0, 1, 255, min_present, max_absent)
        if rep:
            count_only.append(s)
    run = {"min_present": min_present, "max_absent": max_absent, "n_selected": m,
           "count_only_ms_median": round(statistics.median(count_only) * 1e3, 3), "count_only_ms_best": round(min(count_only) * 1e3, 3),
           "count_only_ms_worst": round(max(count_only) * 1e3, 3), "ops": {}}
    for op in ops:
        secs = []
        for rep in range(6):
            hist.zero_()
            torch.cuda.synchronize()
            s = _lib.extract_table_device(ptrs, P, n, 1, 255, min_present, max_absent, op, out.data_ptr(), hist.data_ptr())
            if rep:
                secs.append(s)
        want = reference_table(tabs, op, mask)
        want_hist = torch.bincount(want[want > 0].to(torch.int64), minlength=256)
        exact = bool(torch.equal(out, want)) and bool(torch.equal(hist[1:], want_hist[1:])) and int(hist[0]) == 0
        nonzero = int(hist[1:].sum())
        del want, want_hist
        med = statistics.median(secs)
        run["ops"][op] = {"table_ms_median": round(med * 1e3, 3), "table_ms_best": round(min(secs) * 1e3, 3), "table_ms_worst": round(max(secs) * 1e3, 3),
                          "exact": exact, "nonzero_bytes": nonzero, "ratio_to_count_only": round(med / statistics.median(count_only), 3),
                          "effective_TBps": round((P + A + 2) * n / med / 1e12, 3)}
        assert nonzero == m, (op, nonzero, m)
    return run


def main():
    argv = sys.argv[1:]
    ops = None
    if "--table" in argv:
        at = argv.index("--table")
        ops = _lib.TABLE_OPS if argv[at + 1] == "all" else (argv[at + 1],)
        assert all(op in _lib.TABLE_OPS for op in ops), f"--table takes one of {_lib.TABLE_OPS} or all"
        del argv[at:at + 2]
    path = argv[0] if argv else os.path.join(ROOT, "profiles", "extract_table_k15_n13.json" if ops else "extract_k15_n13.json")
    tabs = genome_tables(P + A, 40_000_000)
    ptrs = [t.data_ptr() for t in tabs]
    acc = torch.zeros((P + A) ** 2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    scan = []
    for rep in range(6):
        s = _lib.gram_device_accumulate(ptrs, n, acc.data_ptr())
        if rep:
            scan.append(s)
    if ops:
        runs = [time_tables(ptrs, tabs, ops, P, 0, reference_mask(tabs, P, 0)), time_tables(ptrs, tabs, ops, 1, A, reference_mask(tabs, 1, A))]
        out = {"kernel": "k_extract_table + k_hist", "device": torch.cuda.get_device_name(0), "kmer_len": 15, "n_present": P, "n_absent": A,
               "table_bytes": n, "bytes_moved_by_the_map": (P + A + 1) * n, "bytes_read_by_the_histogram": n,
               "byte_ratio_to_the_count_pass": round((P + A + 2) / (P + A), 3),
               "pair_scan_ms_median": round(statistics.median(scan) * 1e3, 3), "pair_scan_ms_best": round(min(scan) * 1e3, 3), "runs": runs}
        print(json.dumps(out), flush=True)
        with open(path + ".tmp", "w") as fh:
            json.dump(out, fh, indent=1)
        os.replace(path + ".tmp", path)
        return
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
