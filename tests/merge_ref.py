"""Numpy restatements of the merger's per-slice tallies (pair counts, joint spectra, kWIP's occupancy accumulator) and
kWIP's kernel straight from its definition: the `partial_fn` stand-ins of the CPU tests and the yardsticks of the GPU ones."""
import numpy as np

import oracle
from pykmer_amd import _lib, kwip, spectrum


def oracle_partial(headers, lo, hi, windows, device, threads):
    tabs = [h.read_table_slice(lo, hi) for h in headers]      # a rank reads its slice of every file, nothing else
    N = len(tabs)
    parts = []
    for min_count, max_count in windows:
        m = oracle.gram(tabs, min_count, max_count)
        pair = np.zeros((N, N), np.uint64)
        for i in range(N):
            pair[i, i] = np.count_nonzero((tabs[i] >= min_count) & (tabs[i] <= max_count))
            for j in range(i + 1, N):
                pair[i, j] = m[i, j, 2]
        parts.append(pair)
    return parts


def numpy_spectrum(tabs) -> np.ndarray:
    """The flat accumulator of pk_spectrum_device_accumulate, by np.bincount."""
    N = len(tabs)
    acc = np.zeros(_lib.spectrum_words(N), dtype=np.uint64)
    hist, core = spectrum.split_accumulator(acc, N)
    for i, t in enumerate(tabs):
        hist[i] = np.bincount(t, minlength=256)
    for p, (i, j) in enumerate(spectrum.pair_list(N)):
        core[p] = np.bincount(tabs[i].astype(np.int64) * 256 + tabs[j], minlength=65536).reshape(256, 256)[1:, 1:]
    return acc


def numpy_spectrum_partial(headers, lo, hi, device, threads):
    return numpy_spectrum([h.read_table_slice(lo, hi) for h in headers])


def numpy_occgram(tabs) -> np.ndarray:
    """The flat accumulator of pk_occgram_device_accumulate: np.bincount for occ_hist, masked integer products per class
    (float64 products of u8 counts are exact while a sum stays below 2^53: n * 65025 < 2^53 for any table here)."""
    N = len(tabs)
    acc = np.zeros(_lib.occgram_words(N), dtype=np.uint64)
    occ_hist, lin, gram = kwip.split_accumulator(acc, N)
    X = np.stack([np.asarray(t, dtype=np.uint8) for t in tabs])
    occ = (X > 0).sum(axis=0)
    occ_hist[:] = np.bincount(occ, minlength=N + 1)
    iu = np.triu_indices(N)
    for o in range(1, N + 1):
        sel = X[:, occ == o].astype(np.float64)
        if not sel.shape[1]:
            continue
        lin[o - 1] = sel.sum(axis=1).astype(np.uint64)
        gram[o - 1] = (sel @ sel.T)[iu].astype(np.uint64)
    return acc


def numpy_occgram_partial(headers, lo, hi, device, threads):
    return numpy_occgram([h.read_table_slice(lo, hi) for h in headers])


def direct_kernel(tabs, unweighted=False):
    """K straight from the definition, address by address in float64: sum_x w(o(x)) c_i(x) c_j(x) / (S_i S_j)."""
    N = len(tabs)
    X = np.stack(tabs).astype(np.float64)
    occ = (X > 0).sum(axis=0)
    p = occ / N
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.nan_to_num(-p * np.log2(p) - (1 - p) * np.log2(1 - p))
    if unweighted:
        w = np.ones_like(w)
    s = X.sum(axis=1)
    return (X * w) @ X.T / np.outer(s, s)


# ------------------------------------------------------------------ tables for the merger's kernels
SWEEP9 = [(1, 255), (2, 255), (1, 3), (2, 5), (128, 255), (100, 200), (1, 127), (129, 254), (255, 255)]


def mixed_tables(rng, N, n, density=0.4):
    out = []
    for _ in range(N):
        t = rng.integers(1, 256, size=n, dtype=np.uint8)
        t[rng.random(n) > density] = 0
        t[rng.random(n) < 0.05] = rng.integers(1, 6)          # plenty of small counts for min/max windows
        out.append(t)
    return out


def torch_tables(n, N, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    tabs = []
    for i in range(N):
        t = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
        keep = torch.rand(n, device="cuda", generator=g) < (0.1 + 0.8 * ((i * 7) % N) / N)
        tabs.append(t * keep)
    torch.cuda.synchronize()
    return tabs


def device_bincount(x, bins):
    """torch.bincount's result, by a sort on the device (one hot bin of 10^9 adds would serialise bincount's atomics)."""
    import torch
    vals, counts = torch.unique(x, sorted=True, return_counts=True)
    out = np.zeros(bins, dtype=np.uint64)
    out[vals.cpu().numpy()] = counts.cpu().numpy().astype(np.uint64)
    return out
