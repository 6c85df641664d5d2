"""GPU: the merge kernels at 65 to 128 tables, where nothing else runs them -- k_gram_blk past one LDS opt-in and one launch
(every table-block count NB = 9 ... 16, every shape of the last launch, several tiles per workgroup, the packed-tally worst
case), k_spectrum with 5 to 16 table blocks and ragged last blocks, `merger.py` on 100 tables and its refusal of 129, and
the indexer's device-side table hand-off (pk_indexer_table_device / pk_indexer_table_slice_to_device) into a resident
merge.  Every reference is independent of the kernel under test: the C oracle's pair loop, numpy bincount, exact float64
products on the device."""
import ctypes
import json
import os

import numpy as np
import pytest

import oracle
from pykmer_amd import merger, spectrum
from gpu_support import accumulate_windows, env_without_ranks, run_py
from host_support import write_kin
from merge_ref import SWEEP9, device_bincount, mixed_tables, torch_tables

pytestmark = pytest.mark.gpu
THREADS = max(1, min(16, len(os.sched_getaffinity(0))))

# launch_gram (gram_scan.hip): tables per block, pair blocks per launch, workgroup cap, tiles per workgroup of packed tallies
BLK, MAX_PB, GRID_CAP, MAX_TILES_PER_WG = 8, 24, 1024, 448


def _gram_launches(N):
    """launch_gram's plan for N tables: NB table blocks, NB(NB+1)/2 pair blocks cut into launches of at most MAX_PB, and
    each launch's (pair blocks, slots, packed 16-bit tallies, waves) as its flush() picks them."""
    NB = -(-N // BLK)
    n_pb = NB * (NB + 1) // 2
    sizes = [MAX_PB] * (n_pb // MAX_PB) + ([n_pb % MAX_PB] if n_pb % MAX_PB else [])
    shapes = []
    for m in sizes:
        slots = (1 if N <= 14 else 2) if m <= 3 else 2 if m <= 6 else 1 if m <= 12 else 2
        waves = -(-m // slots)
        if m in (1, 6) and waves < 4:
            waves = 4
        shapes.append((m, slots, m > 16, waves))
    return NB, shapes


def _gram_grid(n):
    """(tiles, workgroups, most tiles of one workgroup) of a k_gram_blk launch over n addresses."""
    tiles = -(-(-(-n // 2048) * 64) // 256)
    grid = min(tiles, GRID_CAP)
    if -(-tiles // grid) > MAX_TILES_PER_WG:
        grid = -(-tiles // MAX_TILES_PER_WG)
    return tiles, grid, -(-tiles // grid)


GRAM_N = [1, 65, 72, 73, 88, 96, 100, 110, 113, 120, 127, 128]
# every table-block count 9 ... 16 and every last-launch remainder they leave (24 = a full last launch), ragged and full blocks
assert sorted({_gram_launches(N)[0] for N in GRAM_N if N > 64}) == list(range(9, 17))
assert {_gram_launches(N)[1][-1][0] for N in GRAM_N if N > 64} == {21, 7, 18, 6, 19, 9, 24, 16}
assert {N % BLK for N in GRAM_N if N > 64} >= {0, 1, 7} and len({N % BLK for N in GRAM_N}) >= 5


def _distinct(tables):
    return len({t.tobytes() for t in tables}) == len(tables)


@pytest.mark.parametrize("N", GRAM_N)
def test_gram_many_tables_vs_oracle(gpu, N):
    """Every entry of every matrix against the oracle's pair loop: all SWEEP9 windows (the SWAR edges 127 / 128 / 129 / 255)
    through pk_gram and through one pk_gram_device_accumulate_windows call, then a ragged size under two windows.  The
    tables are distinct, so a mix-up of table or pair-block indices changes the result; nothing lands below the diagonal."""
    NB, launches = _gram_launches(N)
    assert (N, NB, len(launches)) == (1, 1, 1) or (9 <= NB <= 16 and len(launches) >= 2)
    rng = np.random.default_rng(500 + N)
    for n, windows in ((4 ** 7, SWEEP9), (300_001, [(1, 255), (129, 254)])):
        tables = mixed_tables(rng, N, n)
        assert _distinct(tables)
        acc = accumulate_windows(gpu, tables, windows)
        for w, (mn, mx) in enumerate(windows):
            want = oracle.gram_mt(tables, mn, mx, threads=THREADS)
            assert np.array_equal(gpu.gram(tables, mn, mx), want), (N, n, mn, mx)
            assert np.array_equal(gpu.gram_expand(acc[w]), want), (N, n, mn, mx)
            assert not np.tril(acc[w], -1).any(), (N, n, mn, mx)
            # the totals on their own: the expanded matrix of one table is all zero (merger.py:136 leaves the diagonal out)
            totals = [int(((t >= mn) & (t <= mx)).sum()) for t in tables]
            assert np.diagonal(acc[w]).tolist() == totals, (N, n, mn, mx)
            if N == 1:                                               # one window per call: k_gram_blk, not the multi-window pass
                assert accumulate_windows(gpu, tables, [(mn, mx)])[0].tolist() == [totals], (n, mn, mx)


def test_gram_100_tables_several_tiles_per_workgroup(gpu):
    """N = 100 distinct device tables of 4^12 + a ragged tail: more tiles than the 1024 workgroups, so every workgroup loops
    over tiles in each of the four launches.  Every total and every shared tally of two windows (one with min >= 128)
    against validity matrices multiplied in float64 on the device, chunk by chunk (exact: a chunk holds < 2^53 addresses)."""
    import torch
    torch.cuda.empty_cache()
    N, n = 100, 4 ** 12 + 3 * 2048 + 777
    NB, launches = _gram_launches(N)
    tiles, grid, per_wg = _gram_grid(n)
    assert NB == 13 and len(launches) == 4 and tiles > GRID_CAP and grid == GRID_CAP and per_wg > 1
    tabs = torch_tables(n, N, seed=900)
    ptrs = [t.data_ptr() for t in tabs]
    windows = [(1, 255), (130, 250)]
    acc = torch.zeros((len(windows), N, N), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu.gram_device_accumulate_windows(ptrs, n, acc.data_ptr(), windows)
    got = acc.cpu().numpy().view(np.uint64)
    chunk = 1 << 21
    for w, (mn, mx) in enumerate(windows):
        want = torch.zeros((N, N), dtype=torch.int64, device="cuda")
        for a in range(0, n, chunk):
            v = torch.stack([(t[a:a + chunk] >= mn) & (t[a:a + chunk] <= mx) for t in tabs]).to(torch.float64)
            want += (v @ v.T).to(torch.int64)
            del v
        want = np.triu(want.cpu().numpy()).astype(np.uint64)
        assert np.array_equal(got[w], want), (mn, mx, np.argwhere(got[w] != want)[:8])
    del tabs, acc
    torch.cuda.empty_cache()


@pytest.mark.parametrize("log4n", [15, 16])
def test_gram_packed_tallies_worst_case_128_tables(gpu, log4n):
    """N = 128 dense constant tables: every address valid, so each packed 16-bit tally gets the most a lane can add; at 4^16
    the default grid would give a workgroup more than 448 tiles and the launcher's grid resize runs.  Five buffers are passed
    128 times (aliased pointers cannot show an index mix-up -- test_gram_many_tables_vs_oracle does -- so this checks only
    that no tally carries into its neighbour).  Expected values are closed-form: n where both constants lie in the window."""
    import torch
    torch.cuda.empty_cache()
    N, n = 128, 4 ** log4n
    _, launches = _gram_launches(N)
    tiles, grid, per_wg = _gram_grid(n)
    assert sum(m for m, _, pack, _ in launches if pack) >= 5 * MAX_PB
    assert tiles > GRID_CAP and per_wg >= (128 if log4n == 15 else MAX_TILES_PER_WG)
    if log4n == 16:
        assert -(-tiles // GRID_CAP) > MAX_TILES_PER_WG and grid > GRID_CAP
    bufs = [torch.full((n,), v, dtype=torch.uint8, device="cuda") for v in range(1, 6)]
    torch.cuda.synchronize()
    values = [(i % 5) + 1 for i in range(N)]
    ptrs = [bufs[v - 1].data_ptr() for v in values]
    for mn, mx in ((1, 255), (2, 4)):
        pair, secs = gpu.gram_device_partial(ptrs, n, mn, mx)
        ok = np.array([mn <= v <= mx for v in values])
        want = np.triu(np.outer(ok, ok)).astype(np.uint64) * np.uint64(n)
        assert np.array_equal(pair, want), (log4n, mn, mx, np.argwhere(pair != want)[:8])
    print(f"gram N=128 n=4^{log4n} dense: {secs * 1e3:.1f} ms")
    del bufs
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ joint count spectra, 5 to 16 table blocks --------------
SPEC_N = [20, 33, 42, 47, 59, 64, 70, 85, 100, 128]
assert {N % BLK for N in SPEC_N} == set(range(8)) and {-(-N // BLK) for N in SPEC_N} >= {5, 6, 8, 9, 11, 13, 16}


def _spectrum_tables(rng, N, n):
    """Distinct tables of varying density: uniform counts (most events leave the LDS corner) and Poisson counts of rising
    mean (the (1,1) register tally and the corner); one all-ones table, one all-255 table and, past 40 tables, an empty one."""
    tabs = []
    for i in range(N):
        t = rng.integers(1, 256, n) if i % 2 else np.minimum(rng.poisson(1 + (i % 7) * 6, n), 255)
        tabs.append((t * (rng.random(n) < 0.2 + 0.7 * ((i * 5) % N) / N)).astype(np.uint8))
    tabs[1][:] = 1
    tabs[-1][:] = 255
    if N > 40:
        tabs[N // 2][:] = 0
    return tabs


def _resident_spectrum(gpu, tabs):
    """Host tables -> device tensors -> one pk_spectrum_device_accumulate into an accumulator zeroed on the device -> host."""
    import torch
    dev = [torch.from_numpy(t).cuda() for t in tabs]
    acc = torch.zeros(gpu.spectrum_words(len(tabs)), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu.spectrum_device_accumulate([d.data_ptr() for d in dev], tabs[0].size, acc.data_ptr())
    out = acc.cpu().numpy().view(np.uint64)
    del dev, acc
    return out


@pytest.mark.parametrize("N", SPEC_N)
def test_spectrum_many_tables_vs_bincount(gpu, N):
    """Every histogram and every pair's joint bins against numpy bincount, pair row by pair row (the accumulator is 4.2 GB at
    N = 128: no second one is built)."""
    import torch
    torch.cuda.empty_cache()
    rng = np.random.default_rng(700 + N)
    for n in (2047, 4 ** 7 + 17):
        tabs = _spectrum_tables(rng, N, n)
        assert _distinct(tabs)
        hist, core = spectrum.split_accumulator(_resident_spectrum(gpu, tabs), N)
        for i, t in enumerate(tabs):
            assert np.array_equal(hist[i], np.bincount(t, minlength=256)), (N, n, i)
        p = 0
        for i in range(N - 1):
            m = N - i - 1                                                # the pairs (i, i+1 ... N-1), consecutive in core
            key = np.arange(m, dtype=np.int64)[:, None] * 65536 + tabs[i].astype(np.int64) * 256 + np.stack(tabs[i + 1:])
            want = np.bincount(key.ravel(), minlength=m * 65536).reshape(m, 256, 256)[:, 1:, 1:].astype(np.uint64)
            same = (core[p:p + m] == want).all(axis=(1, 2))
            assert same.all(), (N, n, i, [i + 1 + int(j) for j in np.flatnonzero(~same)[:8]])
            p += m
        assert p == len(core)
        torch.cuda.empty_cache()


def test_spectrum_47_tables_several_chunks_per_lane(gpu):
    """N = 47 (six blocks, the last of 7 tables) at 4^12 + 17 bytes: more 16-byte chunks than the persistent grid has lanes,
    so every lane takes several.  Histograms against pk_table_stats, the marginals of every joint spectrum against them
    (expand refuses a spectrum whose bins exceed its histograms), 16 windows derived by spectrum.window_pairs against
    pk_gram_device_accumulate_windows entry by entry, and a spread of pairs against a bincount on the device."""
    import torch
    torch.cuda.empty_cache()
    N, n = 47, 4 ** 12 + 17
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert -(-n // 16) > 512 * n_cu and -(-N // BLK) == 6 and N % BLK == 7
    g = torch.Generator(device="cuda").manual_seed(47)
    tabs = []
    for i in range(N):
        small = torch.randint(1, 4 + i % 5, (n,), dtype=torch.uint8, device="cuda", generator=g)
        big = torch.randint(1, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
        t = torch.where(torch.rand(n, device="cuda", generator=g) < 0.03, big, small)
        tabs.append(t * (torch.rand(n, device="cuda", generator=g) < 0.05 + 0.9 * ((i * 11) % N) / N))
        del small, big
    ptrs = [t.data_ptr() for t in tabs]
    acc = torch.zeros(gpu.spectrum_words(N), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu.spectrum_device_accumulate(ptrs, n, acc.data_ptr())
    hist, joint = spectrum.expand_accumulator(acc.cpu().numpy().view(np.uint64), N, n)
    del acc
    for i in range(N):
        assert np.array_equal(hist[i], gpu.table_stats(tabs[i].cpu().numpy())), i
    for p, (i, j) in enumerate(spectrum.pair_list(N)):
        assert int(joint[p].sum()) == n
        assert np.array_equal(joint[p].sum(axis=1), hist[i]) and np.array_equal(joint[p].sum(axis=0), hist[j]), (i, j)
    wins = [(1, 255), (2, 255), (1, 3), (2, 5), (1, 1), (255, 255), (3, 255), (1, 2),
            (128, 255), (100, 200), (1, 127), (129, 254), (2, 2), (3, 3), (4, 50), (1, 50)]
    dev = torch.zeros((len(wins), N, N), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu.gram_device_accumulate_windows(ptrs, n, dev.data_ptr(), wins)
    want = dev.cpu().numpy().view(np.uint64)
    for w, got in enumerate(spectrum.window_pairs(hist, joint, wins)):
        assert np.array_equal(got, want[w]), wins[w]
    for i, j in ((0, 1), (0, 46), (7, 8), (15, 40), (39, 40), (40, 46), (45, 46)):
        p = i * N - i * (i + 1) // 2 + (j - i - 1)
        b = device_bincount(tabs[i].to(torch.int32) * 256 + tabs[j].to(torch.int32), 65536)
        assert np.array_equal(joint[p], b.reshape(256, 256)), (i, j)
    del tabs, dev
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ merger.py on 100 tables, and 129 refused --------------
def test_merger_cli_100_tables_and_refuses_129(gpu, tmp_path):
    """100 distinct .kin files at k = 7 (the oracle stands in for the indexer): a four-window sweep writes four .kma, each
    equal to the oracle's pair loop, and .kma.json lists the 100 inputs in order.  129 files: the pair path and --spectrum
    stop with the 128-table limit before any table is read or staged (the Python refusal, not the library's), no output."""
    import synth
    k = 7
    kins, tables = [], []
    for i in range(129):
        fa, _ = synth.family(i, 20_000)
        w = write_kin(tmp_path, f"m{i:03d}.fa", fa.tobytes(), k)
        kins.append(w.path)
        tables.append(w.table)
    assert _distinct(tables)
    proj = str(tmp_path / "p100")
    run_py("merger.py", proj, *kins[:100], "--sweep", "1-255,2-255,1-3,2-5", cwd=str(tmp_path), env=env_without_ranks())
    for mn, mx in ((1, 255), (2, 255), (1, 3), (2, 5)):
        name = f"{proj}.{mn:03d}-{mx:03d}.kma"
        assert np.array_equal(np.load(name)["matrix"], oracle.gram_mt(tables[:100], mn, mx, threads=THREADS)), (mn, mx)
        data = json.load(open(name + ".json"))["data"]
        assert [d["pos"] for d in data] == list(range(100))
        assert [os.path.basename(str(d["index_file"])) for d in data] == [os.path.basename(p) for p in kins[:100]]

    for extra, msg in (((), "a pair tally takes 1 to 128 tables"), (("--spectrum",), "a spectrum takes 2 to 128 tables")):
        proj = str(tmp_path / ("p129" + "".join(extra).replace("-", "_")))
        r = run_py("merger.py", proj, *kins, *extra, cwd=str(tmp_path), status=1, env=env_without_ranks())
        assert msg in r.stderr, (extra, r.stdout[-1000:], r.stderr[-2000:])
        assert "verifying" in r.stdout and "saving" not in r.stdout
        assert not [f for f in os.listdir(tmp_path) if f.startswith(os.path.basename(proj))], extra


# ------------------------------------------------------------------ indexer tables handed over on the device --------------
def _download(gpu, ptr, n):
    out = np.empty(n, dtype=np.uint8)
    gpu._check(gpu.load().pk_dev_download(out.ctypes.data, ctypes.c_void_p(ptr), n, 0))
    return out


def test_indexer_tables_to_resident_merge(gpu):
    """Six genomes counted by _lib.Indexer: pk_indexer_table_device points at the table table_to_host returns (and the
    oracle counts); pk_indexer_table_slice_to_device copies exactly the bytes asked for, at offsets 0, 1, an odd middle one
    and the last byte, and none for an empty slice, and refuses a slice outside the table and any call before finish.
    merger.pair_matrix over ResidentTables -- the live indexer tables, copies assembled from two slices, and one rank's
    address slice copied on its own -- against the oracle."""
    import synth
    k, N = 9, 6
    n = 4 ** k
    guard = 64
    ixs, host, copies = [], [], []
    try:
        for i in range(N):
            fa, _ = synth.family(i, 50_000)
            ix = gpu.Indexer(k)
            ixs.append(ix)
            probe = gpu.DeviceBuffer(64)
            try:
                with pytest.raises(gpu.PkError, match="finish"):
                    ix.table_device_ptr()
                with pytest.raises(gpu.PkError, match="finish"):
                    ix.table_slice_to_device(probe.ptr, 0, 16)
            finally:
                probe.free()
            ix.feed(fa)
            ix.finish()
            table = ix.table_to_host()
            assert np.array_equal(table, oracle.count_fasta(fa, k)["table"]), i
            ptr = ix.table_device_ptr()
            assert ptr % 16 == 0 and np.array_equal(_download(gpu, ptr, n), table), i
            host.append(table)

            for off, ln in ((0, 4096), (1, 4097), (n // 2 + 12_345, 777), (n - 1, 1), (n // 3, 0), (0, n)):
                buf = gpu.DeviceBuffer(ln + 2 * guard)
                try:
                    buf.upload(np.full(buf.n, 0xA5, np.uint8))
                    ix.table_slice_to_device(buf.ptr + guard, off, ln)
                    got = buf.download()
                    assert np.array_equal(got[guard:guard + ln], table[off:off + ln]), (i, off, ln)
                    assert (got[:guard] == 0xA5).all() and (got[guard + ln:] == 0xA5).all(), (i, off, ln)
                finally:
                    buf.free()
            spare = gpu.DeviceBuffer(n + 2 * guard)
            try:
                for off, ln in ((n, 1), (n - 10, 11), (n + 1, 0), (0, n + 1)):
                    with pytest.raises(ValueError, match="outside the table"):
                        ix.table_slice_to_device(spare.ptr, off, ln)
            finally:
                spare.free()

            half = n // 2 + 7
            c = gpu.DeviceBuffer(n)
            copies.append(c)
            ix.table_slice_to_device(c.ptr, 0, half)
            ix.table_slice_to_device(c.ptr + half, half, n - half)
            assert np.array_equal(c.download(), table), i
        assert _distinct(host)

        windows = [(1, 255), (2, 7)]
        want = [oracle.gram(host, mn, mx) for mn, mx in windows]
        for label, ptrs in (("indexer tables", [ix.table_device_ptr() for ix in ixs]), ("copies", [c.ptr for c in copies])):
            tabs = [merger.ResidentTable(p, n, n, device=0) for p in ptrs]
            got = merger.pair_matrix(tabs, windows, devices=(0,))
            for w in range(len(windows)):
                assert np.array_equal(gpu.gram_expand(got[w]), want[w]), (label, windows[w])

        lo, hi = merger.address_slice(n, 2, 3)
        parts = [gpu.DeviceBuffer(hi - lo) for _ in ixs]
        copies += parts
        for ix, b in zip(ixs, parts):
            ix.table_slice_to_device(b.ptr, lo, hi - lo)
        tabs = [merger.ResidentTable(b.ptr, hi - lo, n, device=0, first=lo) for b in parts]
        got = merger.gpu_partial(tabs, lo, hi, windows, 0, 1)
        for w, (mn, mx) in enumerate(windows):
            assert np.array_equal(gpu.gram_expand(got[w]), oracle.gram([t[lo:hi] for t in host], mn, mx)), (mn, mx)
    finally:
        for c in copies:
            c.free()
        for ix in ixs:
            ix.close()
