"""GPU: the merge-side kernels on slices of more than 2^32 bytes whose content depends on the address.

One layout (segment_ref.layout): n = 2^32 + 2^22 + 37; eight blocks of 2^29 bytes and a tail, each with a value vector of
its own in 13 tables, and two dozen single bytes planted around 2^31, around 2^32, at n - 38, at n - 1 and at block
borders.  A byte offset cut to 32 bits reads the head of the tables again (segment_ref.fold), an index that stops at 2^31
reads nothing behind it (segment_ref.clip); before any launch every test asserts on the host that either would change
every result checked here, in every window and for every table.  The tables are block fills on the device, nothing of
their size crosses PCIe, and every expected value is segment_ref's closed form (checked on the CPU against the numpy
yardsticks on the same layout at 1/2^20 of its size).  N = 17 and N = 41 alias the 13 buffers, table i reading buffer
i mod 13: no kernel here refuses aliased pointers, and equal tables are what the closed forms assume.  Peak HBM is the
13 tables (52 GiB) plus one 4 GiB output table or occupancy scratch."""
import functools
import time

import numpy as np
import pytest

import segment_ref as sr

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@functools.lru_cache(maxsize=None)
def _layouts():
    segs, n, at = sr.layout()
    sparse, n2, at2 = sr.layout(sparse_present=sr.EXTRACT["P"])
    assert (n, at) == (n2, at2) and n == 2 ** 32 + 2 ** 22 + 37
    return segs, sparse, n, at


@functools.lru_cache(maxsize=None)
def _want():
    """The references of the true layout -- after the precondition: a kernel that folds at 2^32 or clips at 2^31 gives
    another answer for every one of them."""
    segs, sparse, _, _ = _layouts()
    true = sr.results(segs, sparse)
    sr.assert_visible(true, sr.results(sr.fold(segs, 2 ** 32), sr.fold(sparse, 2 ** 32)), "fold at 2^32")
    sr.assert_visible(true, sr.results(sr.clip(segs, 2 ** 31), sr.clip(sparse, 2 ** 31)), "clip at 2^31")
    return true


class _Tables:
    """The tables `idx` of a layout as torch tensors in HBM, filled segment by segment; .ptrs(N) aliases them over N tables."""

    def __init__(self, segs, n, idx):
        import torch
        torch.cuda.empty_cache()
        self.t0 = time.perf_counter()
        self.tabs = []
        for i in idx:
            t = torch.empty(n, dtype=torch.uint8, device="cuda")
            for s, e, v in segs:
                t[s:e].fill_(int(v[i]))
            self.tabs.append(t)
        torch.cuda.synchronize()
        for t, i in zip(self.tabs, idx):                     # the fills did what the segment list says
            assert int(t.sum(dtype=torch.int64).item()) == sum((e - s) * int(v[i]) for s, e, v in segs), i
        self.fill_seconds = time.perf_counter() - self.t0

    def ptrs(self, N=None):
        N = len(self.tabs) if N is None else N
        return [self.tabs[i % len(self.tabs)].data_ptr() for i in range(N)]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        import torch
        self.tabs = []
        torch.cuda.empty_cache()
        print(f"  tables: {self.fill_seconds:.2f} s to fill, {time.perf_counter() - self.t0:.2f} s in all")


def _base(n_tables=sr.N_BASE):
    segs, _, n, _ = _layouts()
    return _Tables(segs, n, range(n_tables))


def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), (what, np.argwhere(got != want)[:5], got[got != want][:5], want[got != want][:5])


@pytest.mark.parametrize("N,windows", sr.PAIR_RUNS)
def test_pair_scan_past_4gib(gpu, N, windows):
    """k_gram_blk: its unpacked shape at N = 13, the packed 16-bit tallies at N = 41."""
    want, n = _want(), _layouts()[2]
    with _base() as tabs:
        for w in windows:
            pair, secs = gpu.gram_device_partial(tabs.ptrs(N), n, *w)
            _same(pair, want["pair", N, w], (N, w))
            print(f"  gram N={N} {w}: kernel {secs * 1e3:.2f} ms")


@pytest.mark.parametrize("N,W", sr.SWEEP_RUNS)
def test_window_sweep_past_4gib(gpu, N, W):
    """k_gram_mw in its three kernel shapes, one pass each: fetch_item's scalar base plus 32-bit lane offset, and the
    load_word path of the last, partial tile."""
    import torch
    want, n = _want(), _layouts()[2]
    windows = sr.SWEEP_WINDOWS[:W]
    with _base(min(N, sr.N_BASE)) as tabs:
        acc = torch.zeros((W, N, N), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        secs = gpu.gram_device_accumulate_windows(tabs.ptrs(N), n, acc.data_ptr(), windows)
        got = acc.cpu().numpy().view(np.uint64)
        del acc
        for w, win in enumerate(windows):
            _same(got[w], want["sweep", N, win], (N, win))
        print(f"  sweep N={N} W={W}: kernel {secs * 1e3:.2f} ms")


def test_spectrum_past_4gib(gpu):
    import torch
    want, n = _want(), _layouts()[2]
    with _base() as tabs:
        acc = torch.zeros(gpu.spectrum_words(sr.N_BASE), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        secs = gpu.spectrum_device_accumulate(tabs.ptrs(), n, acc.data_ptr())
        got = acc.cpu().numpy().view(np.uint64)
        del acc
        _same(got, want["spectrum", sr.N_BASE], "spectrum")
        print(f"  spectrum N=13: kernel {secs * 1e3:.2f} ms")


@pytest.mark.parametrize("N", sr.OCC_RUNS)
def test_occgram_past_4gib(gpu, N):
    """N = 13 is one pass in registers; N = 17 takes several passes over the occupancy bytes kept in a scratch of n bytes."""
    import torch
    want, n = _want(), _layouts()[2]
    with _base() as tabs:
        acc = torch.zeros(gpu.occgram_words(N), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        secs = gpu.occgram_device_accumulate(tabs.ptrs(N), n, acc.data_ptr())
        got = acc.cpu().numpy().view(np.uint64)
        del acc
        _same(got, want["occgram", N], ("occgram", N))
        print(f"  occgram N={N}: kernel {secs * 1e3:.2f} ms")


@pytest.mark.parametrize("N,windows", sr.PATTERN_RUNS)
def test_patterns_past_4gib(gpu, N, windows):
    """N = 13 is one launch, N = 15 two."""
    import torch
    want, n = _want(), _layouts()[2]
    with _base() as tabs:
        for w in windows:
            acc = torch.zeros(1 << N, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            secs = gpu.patterns_device_accumulate(tabs.ptrs(N), n, acc.data_ptr(), *w)
            got = acc.cpu().numpy().view(np.uint64)
            del acc
            _same(got, want["patterns", N, w], (N, w))
            print(f"  patterns N={N} {w}: kernel {secs * 1e3:.2f} ms")


def _condition():
    e = sr.EXTRACT
    return e["tables"], e["P"], (e["mn"], e["mx"], e["min_present"], e["max_absent"])


def test_extract_sparse_past_4gib(gpu):
    """The sparse variant: the blocks are 0 in the present tables, so only plants select.  addr and counts of the whole
    slice (the masks[off / 16] index and the scan over 2^18 workgroup counts run past 2^32 addresses), then of a sub-slice
    that starts 16 bytes above 2^32 with first_addr to match."""
    import torch
    want = _want()
    _, sparse, n, at = _layouts()
    idx, P, cond = _condition()
    addr, counts = want["extract", "addr"], want["extract", "counts"]
    assert 6 <= addr.size < len(at) and (addr >= 2 ** 32).sum() >= 2 and (addr < 2 ** 31).sum() >= 2
    assert n // 16384 > 2 ** 18                              # 256 rounds of the 1024-thread scan over the workgroup counts
    start = 2 ** 32 + 16
    keep = addr >= start
    assert 2 <= keep.sum() < addr.size
    sub = sr.extract_rows(sr.restrict(sr.tables_of(sparse, idx), start, n), P, *cond, first_addr=start)
    assert np.array_equal(sub[0], addr[keep]) and np.array_equal(sub[1], counts[keep])
    with _Tables(sparse, n, idx) as tabs:
        for first, size, w_addr, w_counts in ((0, n, addr, counts), (start, n - start, sub[0], sub[1])):
            cap = w_addr.size + 3
            out_a = torch.full((cap * 8,), SENTINEL, dtype=torch.uint8, device="cuda")
            out_c = torch.full((max(16, cap * P),), SENTINEL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            m, fits, secs = gpu.extract_device([p + first for p in tabs.ptrs()], P, size, first, *cond, out_a.data_ptr(), out_c.data_ptr(), cap)
            assert (m, fits) == (w_addr.size, True), (first, m, fits, w_addr.size)
            got_a, got_c = out_a.cpu().numpy(), out_c.cpu().numpy()
            _same(got_a[:m * 8].view(np.uint64), w_addr, ("addr", first))
            _same(got_c[:m * P].reshape(m, P), w_counts, ("counts", first))
            assert (got_a[m * 8:] == SENTINEL).all() and (got_c[m * P:] == SENTINEL).all(), first
            del out_a, out_c
            print(f"  extract sparse from {first}: {m} rows, kernels {secs * 1e3:.2f} ms")


def test_extract_dense_count_past_4gib(gpu):
    """The dense layout, count-only: whole blocks on either side of 2^31 select."""
    want = _want()
    segs, _, n, _ = _layouts()
    idx, P, cond = _condition()
    with _Tables(segs, n, idx) as tabs:
        m, fits, secs = gpu.extract_device(tabs.ptrs(), P, n, 0, *cond)
        assert (m, fits) == (int(want["extract", "dense"][0]), False) and m > 2 ** 29
        print(f"  extract dense: {m} selected, kernels {secs * 1e3:.2f} ms")


@pytest.mark.parametrize("op", ["sum", "min", "max", "count"])
def test_extract_table_past_4gib(gpu, op):
    """k_extract_table's output of n bytes: its histogram by the histogram pass that table_stats runs, taken where the
    table is (a 4 GiB download is what this file avoids), and 4 KiB downloaded around every block border and every
    planted byte, byte for byte; the bytes behind n are untouched."""
    import torch
    want = _want()
    segs, _, n, at = _layouts()
    idx, P, cond = _condition()
    out_segs, hist256 = sr.table(sr.tables_of(segs, idx), P, op, *cond)
    assert np.array_equal(hist256, want["table", op]) and np.count_nonzero(hist256) >= 2
    with _Tables(segs, n, idx) as tabs:
        out = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        hist = torch.zeros(256, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        secs = gpu.extract_table_device(tabs.ptrs(), P, n, *cond, op, out.data_ptr(), hist.data_ptr())
        h = hist.cpu().numpy().view(np.uint64).copy()
        assert h[0] == 0                                     # the device tallies the values 1 .. 255
        h[0] = n - int(h[1:].sum())
        _same(h, hist256, ("hist256", op))
        for x in sorted(set(at) | {b << 29 for b in range(1, 9)} | {n - 1}):
            lo, hi = max(0, x - 2048), min(n, x + 2048)
            _same(out[lo:hi].cpu().numpy(), sr.window_bytes(out_segs, lo, hi), (op, x))
        assert (out[n:].cpu().numpy() == SENTINEL).all(), op
        del out, hist
        print(f"  extract table {op}: kernels {secs * 1e3:.2f} ms")
