"""Times k_occgram (pk_occgram_device_accumulate) on tables of 4^15 bytes resident in HBM, each time set against ONE
single-window scan (pk_gram_device_partial) of the same tables.  Kernel seconds from HIP events: median (and best) of 5
after 1 warm-up.  Table sets, the ones tools/bench_spectrum.py uses (N = 13 unless noted):
  genome        synth.family(i, 40_000_000) counted by the indexer (the bench's merge set)      also at N = 32
  dense_genome  synth.family(i, 400_000_000)
  coverage      40 % non-zero, counts Poisson(30) clipped to 255
  uniform       40 % non-zero, counts uniform 1..255 (tools/bench_gram.py)
Per set it also records the class mix the kernel's cost depends on: the mean number of distinct non-zero occupancies per
256 and per 1024 addresses (a tile group).  Every pass is checked: occ_hist sums to 4^15 and sum_o lin[o][i] equals the
table's sum.  Writes one JSON line per set to stdout and all of them to profiles/kwip_n13.json (or the path given as the
first argument; a second argument picks sets by name)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_spectrum import genome_tables, n, random_tables  # noqa: E402
from pykmer_amd import _lib, kwip  # noqa: E402


def class_mix(tabs, N):
    occ = torch.zeros(n, dtype=torch.int16, device="cuda")
    for t in tabs:
        occ += (t > 0)
    out = {}
    for span in (256, 1024):
        o = occ.view(-1, span).to(torch.int64)
        present = torch.zeros((o.shape[0], N + 1), dtype=torch.bool, device="cuda")
        present.scatter_(1, o, True)
        out[f"classes_per_{span}"] = round(float(present[:, 1:].sum(dim=1).double().mean()), 3)
    del occ
    return out


def measure(name, tabs):
    N = len(tabs)
    ptrs = [t.data_ptr() for t in tabs]
    acc = torch.zeros(_lib.occgram_words(N), dtype=torch.int64, device="cuda")
    occ_t, scan_t = [], []
    for rep in range(6):
        acc.zero_()
        torch.cuda.synchronize()
        s = _lib.occgram_device_accumulate(ptrs, n, acc.data_ptr())
        _, g = _lib.gram_device_partial(ptrs, n)
        if rep:
            occ_t.append(s)
            scan_t.append(g)
    occ_hist, lin, gram = kwip.split_accumulator(acc.cpu().numpy().view(np.uint64), N)
    exact = int(occ_hist.sum()) == n
    for i, t in enumerate(tabs):
        exact &= int(lin[:, i].sum()) == int(t.sum(dtype=torch.int64))
    out = {"set": name, "N": N, "table_bytes": n, "nonzero_fraction": round(float(occ_hist[1:].sum()) / n, 4), **class_mix(tabs, N),
           "occgram_ms_median": round(statistics.median(occ_t) * 1e3, 3), "occgram_ms_best": round(min(occ_t) * 1e3, 3),
           "scan_ms_median": round(statistics.median(scan_t) * 1e3, 3), "scan_ms_best": round(min(scan_t) * 1e3, 3),
           "ratio_median": round(statistics.median(occ_t) / statistics.median(scan_t), 2), "exact": bool(exact)}
    print(json.dumps(out), flush=True)
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kwip_n13.json")
    only = set(sys.argv[2].split(",")) if len(sys.argv) > 2 else None
    sets = [("genome", lambda: genome_tables(13, 40_000_000)), ("dense_genome", lambda: genome_tables(13, 400_000_000)),
            ("coverage", lambda: random_tables(13, "coverage")), ("uniform", lambda: random_tables(13, "uniform")),
            ("genome_n32", lambda: genome_tables(32, 40_000_000))]
    results = []
    for name, make in sets:
        if only and name not in only:
            continue
        tabs = make()
        results.append(measure(name, tabs))
        del tabs
        torch.cuda.empty_cache()
    with open(path + ".tmp", "w") as fh:
        json.dump({"kernel": "k_occgram", "device": torch.cuda.get_device_name(0), "results": results}, fh, indent=1)
    os.replace(path + ".tmp", path)


if __name__ == "__main__":
    main()
