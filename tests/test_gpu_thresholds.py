"""GPU: every count threshold t = 1 .. 255 as the windows (t, 255), (1, t) and (t, t) -- 765 windows -- through every
bit-trick window comparator of the merge side: valid_bits (k_gram_blk, FAST and general), bit_transpose8 + planes_ge
(k_gram_mw), pt_valid (k_patterns) and x_ge / x_valid (k_extract_count, k_extract_table).  The tables hold every byte
value at every offset of a 2 KiB word group (segment_ref.threshold_tables, its coverage checked on the CPU), so every
byte lane of every comparator meets every value on both sides of every threshold.  The yardstick is the window rule as
written, (t >= mn) & (t <= mx), on the whole tables (threshold_ref); all comparisons are exact."""
import functools
import time

import numpy as np
import pytest

import segment_ref as sr
import threshold_ref as tr

pytestmark = pytest.mark.gpu

N_MAX, SIZE = 33, 1 << 19
LISTS = dict(zip(("from_t", "up_to_t", "only_t"), sr.threshold_windows()))


@functools.lru_cache(maxsize=None)
def _host_tables():
    return tuple(sr.threshold_tables(N_MAX, SIZE, seed=765))


def _tables(N):
    """(N, SIZE) uint8 tensor in HBM -- the first N of the same 33 tables -- and the pointers of its rows."""
    import torch
    T = tr.stack(_host_tables()[:N], "cuda")
    torch.cuda.synchronize()
    return T, [T[i].data_ptr() for i in range(N)]


@pytest.mark.parametrize("which", sorted(LISTS))
@pytest.mark.parametrize("N", [5, 13, 20, 30, 33])
def test_pair_tallies_at_every_threshold(gpu, N, which):
    """One gram_device_accumulate_windows call of 255 windows, the call's maximum (so the `out` byte of k_gram_mw's
    WindowSet runs up to 254).  N = 5, 13, 20 and 30 are the four shapes of k_gram_mw, in passes of 8, 8, 5 and 3 windows
    sorted by their lower bound (255 = 31 x 8 + 7 = 51 x 5 = 85 x 3: the last pass of a call is a sweep pass too, a
    single-window leftover is test_window_sweep_in_one_pass_vs_oracle's case); N = 33 has no sweep pass and runs 255 single scans of k_gram_blk, the FAST valid_bits
    for (1, 255) and the general one for the rest.  Every entry of every N x N matrix is compared."""
    import torch
    windows = LISTS[which]
    T, ptrs = _tables(N)
    acc = torch.zeros((len(windows), N, N), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    secs = gpu.gram_device_accumulate_windows(ptrs, SIZE, acc.data_ptr(), windows)
    t1 = time.perf_counter()
    got = acc.cpu().numpy().view(np.uint64)
    bad = [(mn, mx) for w, (mn, mx) in enumerate(windows) if not np.array_equal(got[w], tr.pair(tr.masks(T, mn, mx)))]
    print(f"  N={N} {which}: kernels {secs * 1e3:.2f} ms, call {t1 - t0:.2f} s, yardstick {time.perf_counter() - t1:.2f} s")
    assert not bad, (N, which, len(bad), bad[:8])


@pytest.mark.parametrize("N", [3, 12])
def test_patterns_at_every_threshold(gpu, N):
    """pt_valid under all 765 windows, one launch each; at N = 12 the tables fill the `lo` and the `hi` dwords."""
    import torch
    T, ptrs = _tables(N)
    windows = [w for ws in LISTS.values() for w in ws]
    acc = torch.zeros((len(windows), 1 << N), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for w, (mn, mx) in enumerate(windows):
        gpu.patterns_device_accumulate(ptrs, SIZE, acc[w].data_ptr(), mn, mx)
    got = acc.cpu().numpy().view(np.uint64)
    bad = [(mn, mx) for w, (mn, mx) in enumerate(windows) if not np.array_equal(got[w], tr.patterns(tr.masks(T, mn, mx)))]
    assert not bad, (N, len(bad), bad[:8])


def test_extract_counts_at_every_threshold(gpu):
    """x_ge / x_valid in k_extract_count under all 765 windows, count-only: 3 present tables, 2 absent ones."""
    T, ptrs = _tables(5)
    bad = []
    for ws in LISTS.values():
        for mn, mx in ws:
            m, fits, _ = gpu.extract_device(ptrs, 3, SIZE, 0, mn, mx, 2, 1)
            want = int(tr.selection(tr.masks(T[:3], mn, mx), T[3:], 2, 1).sum().item())
            if m != want or fits != (want == 0):
                bad.append((mn, mx, m, want))
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("op", ["sum", "count"])
def test_extract_tables_at_every_threshold(gpu, op):
    """x_valid in k_extract_table under all 765 windows, 3 present tables: every byte of every output table, and its
    histogram of the values 1 .. 255."""
    import torch
    T, ptrs = _tables(3)
    out = torch.empty(SIZE, dtype=torch.uint8, device="cuda")
    hist = torch.zeros(256, dtype=torch.int64, device="cuda")
    bad = []
    for ws in LISTS.values():
        for mn, mx in ws:
            out.fill_(0xA5)
            hist.zero_()
            torch.cuda.synchronize()
            gpu.extract_table_device(ptrs, 3, SIZE, mn, mx, 2, 0, op, out.data_ptr(), hist.data_ptr())
            m = tr.masks(T, mn, mx)
            want = tr.table(T, m, tr.selection(m, T[:0], 2, 0), op)
            h = torch.bincount(want.to(torch.int64), minlength=256)
            h[0] = 0
            if not (torch.equal(out, want) and torch.equal(hist, h)):
                bad.append((mn, mx))
    assert not bad, (op, len(bad), bad[:8])
