"""Times k_spectrum (pk_spectrum_device_accumulate) on tables of 4^15 bytes resident in HBM, each time set against ONE
single-window scan (pk_gram_device_partial) of the same tables.  Kernel seconds from HIP events: best and median of 5
after 1 warm-up.  Table sets (N = 13 unless noted):
  genome        synth.family(i, 40_000_000) counted by the indexer (the bench's merge set)      also at N = 32
  dense_genome  synth.family(i, 400_000_000)
  coverage      40 % non-zero, counts Poisson(30) clipped to 255
  uniform       40 % non-zero, counts uniform 1..255 (tools/bench_gram.py)
Every pass is also checked: the (1,255) window derived from the spectrum equals the scan's tallies and every pair's joint
spectrum sums to its marginals.  Writes one JSON line per set to stdout and all of them to profiles/spectrum_n13.json
(or the path given as the first argument)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import synth  # noqa: E402
from pykmer_amd import _lib, spectrum  # noqa: E402

K = 15
n = 4 ** K


def genome_tables(N, bp):
    out = []
    with _lib.Indexer(K, device=0) as ix:
        for i in range(N):
            fa, _ = synth.family(i, bp)
            ix.reset()
            ix.feed(fa)
            ix.finish()
            t = torch.empty(n, dtype=torch.uint8, device="cuda")
            ix.table_slice_to_device(t.data_ptr(), 0, n)
            out.append(t)
    torch.cuda.synchronize()
    return out


def random_tables(N, kind):
    g = torch.Generator(device="cuda").manual_seed(7)
    out = []
    for _ in range(N):
        keep = torch.rand(n, device="cuda", generator=g) < 0.4
        if kind == "uniform":
            t = torch.randint(1, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
        else:
            t = torch.poisson(torch.full((n,), 30.0, device="cuda"), generator=g).clamp_(max=255).to(torch.uint8)
        out.append(t * keep)
        del keep, t
    torch.cuda.synchronize()
    return out


def measure(name, tabs):
    N = len(tabs)
    ptrs = [t.data_ptr() for t in tabs]
    acc = torch.zeros(_lib.spectrum_words(N), dtype=torch.int64, device="cuda")
    spec_t, scan_t = [], []
    for rep in range(6):
        acc.zero_()
        torch.cuda.synchronize()
        s = _lib.spectrum_device_accumulate(ptrs, n, acc.data_ptr())
        pair, g = _lib.gram_device_partial(ptrs, n)
        if rep:
            spec_t.append(s)
            scan_t.append(g)
    hist, joint = spectrum.expand_accumulator(acc.cpu().numpy().view(np.uint64), N, n)
    exact = bool(np.array_equal(spectrum.window_pairs(hist, joint, [(1, 255)])[0], pair))
    for p, (i, j) in enumerate(spectrum.pair_list(N)):
        exact &= bool(np.array_equal(joint[p].sum(axis=1), hist[i]) and np.array_equal(joint[p].sum(axis=0), hist[j]))
    nonzero = float(hist[:, 1:].sum()) / (N * n)
    out = {"set": name, "N": N, "table_bytes": n, "nonzero_fraction": round(nonzero, 4),
           "spectrum_ms_best": round(min(spec_t) * 1e3, 3), "spectrum_ms_median": round(statistics.median(spec_t) * 1e3, 3),
           "scan_ms_best": round(min(scan_t) * 1e3, 3), "scan_ms_median": round(statistics.median(scan_t) * 1e3, 3),
           "ratio_best": round(min(spec_t) / min(scan_t), 2), "exact": exact}
    print(json.dumps(out), flush=True)
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "spectrum_n13.json")
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
        json.dump({"kernel": "k_spectrum", "device": torch.cuda.get_device_name(0), "results": results}, fh, indent=1)
    os.replace(path + ".tmp", path)


if __name__ == "__main__":
    main()
