"""GPU: k_patterns (pk_patterns_device_accumulate) against numpy on mixed and adversarial tables at every table count that
changes its path (the lo / hi byte at 8 and 9, the bin limit and the several launches at 14, 15 and 16), its accumulation
over sub-slices and repeats, a bin past 2^32, cross-checks against torch, the pair scan and the occgram pass on the device,
its refusals, and the `merger.py --patterns` command line."""
import json

import numpy as np
import pytest

from pykmer_amd import kwip, merger, patterns
from gpu_support import SENTINEL, SentinelOut, accumulate_windows, env_without_ranks, family_kins, run_py
from merge_ref import device_bincount, mixed_tables, torch_tables
from patterns_ref import numpy_patterns

pytestmark = pytest.mark.gpu

WINDOWS = [(1, 255), (2, 255), (1, 1), (3, 50)]


def _device_patterns(gpu, tabs, windows, cuts=None, start=0, ptrs_of=None, repeats=1):
    """Host tables -> device buffers -> one accumulator of 2^N u64 per window, every word started at `start`; one call per
    window and per (a, b) of `cuts`, `repeats` times over.  ptrs_of(bufs) picks the pointers handed to the library."""
    N, n = len(tabs), tabs[0].size
    words = gpu.patterns_words(N)
    bufs = [gpu.DeviceBuffer(max(16, n)) for _ in (tabs if ptrs_of is None else tabs[:1])]
    acc = gpu.DeviceBuffer(len(windows) * words * 8)
    try:
        for b, t in zip(bufs, tabs):
            b.upload(t)
        acc.upload(np.full(len(windows) * words, start, dtype=np.uint64).view(np.uint8))
        ptrs = [b.ptr for b in bufs] if ptrs_of is None else ptrs_of(bufs)
        for _ in range(repeats):
            for w, (mn, mx) in enumerate(windows):
                for a, b in (cuts or [(0, n)]):
                    secs = gpu.patterns_device_accumulate([p + a for p in ptrs], b - a, acc.ptr + w * words * 8, mn, mx)
                    assert secs >= 0
        return acc.download().view(np.uint64).reshape(len(windows), words).copy()
    finally:
        for b in bufs + [acc]:
            b.free()


def _check(gpu, tabs, windows, what):
    got = _device_patterns(gpu, tabs, windows)
    for g, (mn, mx) in zip(got, windows):
        want = numpy_patterns(tabs, mn, mx)
        assert np.array_equal(g, want), (what, mn, mx, np.flatnonzero(g != want)[:5], g[g != want][:5], want[g != want][:5])
    return got


@pytest.mark.parametrize("N", [1, 2, 7, 8, 9, 13, 14, 15, 16])
def test_patterns_vs_numpy(gpu, N):
    rng = np.random.default_rng(N)
    for n in (1, 15, 31, 2047, 2048, 2049, 3 * 8192 + 1037, 4 ** 8 + 11):
        got = _check(gpu, mixed_tables(rng, N, n), WINDOWS, (N, n))
        assert all(int(g.sum()) == n for g in got)
    assert np.count_nonzero(got[0]) > min(1 << N, 2000) // 2                   # the tables spread over the bins


@pytest.mark.parametrize("N", [5, 16])
def test_patterns_adversarial(gpu, N):
    n = 70_001
    rng = np.random.default_rng(3)
    last = (1 << N) - 1

    def only(got, bins):
        want = np.zeros(1 << N, np.uint64)
        for b, v in bins.items():
            want[b] = v
        return np.array_equal(got, want)
    zero = [np.zeros(n, np.uint8) for _ in range(N)]
    assert only(_check(gpu, zero, [(1, 255)], "zero")[0], {0: n})
    full = [np.full(n, 255, np.uint8) for _ in range(N)]
    got = _check(gpu, full, [(255, 255), (1, 254)], "255")
    assert only(got[0], {last: n}) and only(got[1], {0: n})
    one = rng.integers(0, 256, n).astype(np.uint8)
    got = _check(gpu, [one] * N, WINDOWS, "identical")
    for g in got:
        assert not g[1:last].any() and int(g[0]) + int(g[last]) == n
    same_ptr = _device_patterns(gpu, [one] * N, WINDOWS, ptrs_of=lambda bufs: [bufs[0].ptr] * N)
    assert np.array_equal(same_ptr, got)
    private = []
    for t in range(N):
        tab = np.zeros(n, np.uint8)
        tab[t::N] = rng.integers(1, 256, tab[t::N].size)
        private.append(tab)
    g = _check(gpu, private, [(1, 255)], "private")[0]
    assert int(g[0]) == 0 and sum(int(g[1 << t]) for t in range(N)) == n
    for mn, mx in ((3, 50), (128, 200), (2, 254), (127, 128)):
        edge = [rng.choice(np.array([mn - 1, mn, mx, mx + 1], np.uint8), n) for _ in range(N)]
        _check(gpu, edge, [(mn, mx)], ("edges", mn, mx))
    holed = mixed_tables(rng, N, n)
    holed[N // 2] = np.zeros(n, np.uint8)
    for g in _check(gpu, holed, WINDOWS, "one table zero"):
        assert not g[(np.arange(1 << N) >> (N // 2)) & 1 == 1].any()


def test_patterns_accumulate(gpu):
    rng = np.random.default_rng(11)
    n = 300_001
    for N in (6, 15):
        tabs = mixed_tables(rng, N, n)
        one = _check(gpu, tabs, WINDOWS, N)
        for cut in (2048, 100_352, 100_384 - 32 * 3):
            assert cut % 32 == 0
            assert np.array_equal(_device_patterns(gpu, tabs, WINDOWS, cuts=[(0, cut), (cut, n)]), one), (N, cut)
        assert np.array_equal(_device_patterns(gpu, tabs, WINDOWS, repeats=2), one * np.uint64(2))         # bin 0 doubles too
        start = 0x0123456789ABCDEF
        got = _device_patterns(gpu, tabs, WINDOWS, start=start)
        assert np.array_equal(got, one + np.uint64(start))                                       # added to, not overwritten


def test_patterns_bin_past_2_32(gpu):
    """One all-255 table of 2^32 + 4096 bytes at window 255-255: every address lands in bin 1."""
    import torch
    torch.cuda.empty_cache()
    n = 2 ** 32 + 4096
    a = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    acc = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu.patterns_device_accumulate([a.data_ptr()], n, acc.data_ptr(), 255, 255)
    assert acc.cpu().numpy().view(np.uint64).tolist() == [0, n]
    del a
    torch.cuda.empty_cache()


@pytest.mark.parametrize("N", [13, 16])
def test_patterns_cross_checks_on_device(gpu, N):
    import torch
    n = 4 ** 12
    tabs = torch_tables(n, N, seed=N)
    ptrs = [t.data_ptr() for t in tabs]
    host = None
    for mn, mx in ((1, 255), (3, 50)):
        acc = torch.zeros(1 << N, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        gpu.patterns_device_accumulate(ptrs, n, acc.data_ptr(), mn, mx)
        got = acc.cpu().numpy().view(np.uint64)
        words = torch.zeros(n, dtype=torch.int64, device="cuda")
        for t, tab in enumerate(tabs):
            words |= ((tab >= mn) & (tab <= mx)).to(torch.int64) << t
        assert np.array_equal(got, torch.bincount(words, minlength=1 << N).cpu().numpy().astype(np.uint64)), (mn, mx)
        assert np.array_equal(got, device_bincount(words, 1 << N))
        if host is None:
            host = [t.cpu().numpy() for t in tabs]
        assert np.array_equal(patterns.matrix_from_patterns(got, N), accumulate_windows(gpu, host, [(mn, mx)])[0]), (mn, mx)
        if (mn, mx) == (1, 255):
            occ = torch.zeros(gpu.occgram_words(N), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            gpu.occgram_device_accumulate(ptrs, n, occ.data_ptr())
            occ_hist = kwip.split_accumulator(occ.cpu().numpy().view(np.uint64), N)[0]
            assert np.array_equal(patterns.occupancy_from_patterns(got, N), occ_hist)


def test_patterns_refusals(gpu):
    tab = gpu.DeviceBuffer(4096)
    out = SentinelOut(acc=(1 << 16) * 8)
    try:
        tab.zero()
        for N in (0, 17):
            with pytest.raises(ValueError, match="1 to 16 tables"):
                gpu.patterns_device_accumulate([tab.ptr] * N, 64, out.acc.ptr)
        for mn, mx in ((0, 255), (5, 4), (1, 256)):
            with pytest.raises(ValueError, match="1 <= min <= max <= 255"):
                gpu.patterns_device_accumulate([tab.ptr] * 3, 64, out.acc.ptr, mn, mx)
        with pytest.raises(ValueError, match="null accumulator"):
            gpu.patterns_device_accumulate([tab.ptr] * 3, 64, 0)
        with pytest.raises(ValueError, match="16-byte aligned"):
            gpu.patterns_device_accumulate([tab.ptr, tab.ptr + 8], 64, out.acc.ptr)
        with pytest.raises(ValueError, match="out of range"):
            gpu.patterns_device_accumulate([tab.ptr], 2 ** 40 + 1, out.acc.ptr)
        assert out.untouched()
        gpu.patterns_device_accumulate([tab.ptr] * 3, 64, out.acc.ptr)                           # and a good call is taken
        word = int(np.full(1, SENTINEL, np.uint8).repeat(8).view(np.uint64)[0])
        got = out.acc.download().view(np.uint64)
        assert int(got[0]) == (word + 64) % 2 ** 64 and (got[1:] == word).all()
    finally:
        tab.free()
        out.free()


def test_patterns_command_lines(gpu, tmp_path, manifest, monkeypatch):
    """indexer.py -> merger.py --patterns --sweep on the G7 FASTA inputs: per window the .kmv equals numpy over the tables
    and the .kma a plain merger.py run; the same files from .kin.bgz inputs in forced sub-slices and from two ranks (gloo on
    the one GPU); extract.py selects count_where's number of k-mers."""
    import gzip
    kins = sorted(family_kins(tmp_path, manifest))
    env = env_without_ranks()
    sweep = [(1, 255), (2, 255)]
    proj = str(tmp_path / "pv")
    r = run_py("merger.py", proj, *kins, "--patterns", "--sweep", "1-255,2-255", cwd=str(tmp_path), env=env)
    assert r.stdout.count("saving") == 10
    run_py("merger.py", str(tmp_path / "plain"), *kins, "--sweep", "1-255,2-255", cwd=str(tmp_path), env=env)
    tabs = [merger.Header(k, index_file=k).read_table_slice(0, 4 ** 7) for k in kins]
    N = len(tabs)
    first = {}
    for mn, mx in sweep:
        w = f"{mn:03d}-{mx:03d}"
        first[w] = patterns.load(f"{proj}.{w}.kmv")
        assert np.array_equal(first[w]["patterns"], numpy_patterns(tabs, mn, mx)), w
        with np.load(f"{proj}.{w}.kma") as a, np.load(str(tmp_path / f"plain.{w}.kma")) as b:
            assert a["matrix"].tobytes() == b["matrix"].tobytes() and a["matrix"].dtype == b["matrix"].dtype, w

    bgz = []
    for kin in kins:
        with open(kin, "rb") as fh, gzip.open(kin + ".bgz", "wb") as out:
            out.write(fh.read())
        bgz.append(kin + ".bgz")
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(13 * 4096))
    merger.merge(str(tmp_path / "sub"), sorted(bgz), windows=sweep, patterns=True)
    monkeypatch.delenv("PK_MERGE_HBM_BUDGET")
    run_py("merger.py", str(tmp_path / "two"), *kins, "--patterns", "--sweep", "1-255,2-255", "--gpus", "2", cwd=str(tmp_path),
           env=dict(env, PK_DIST_BACKEND="gloo"))
    for other in ("sub", "two"):
        for w, one in first.items():
            assert np.array_equal(patterns.load(str(tmp_path / f"{other}.{w}.kmv"))["patterns"], one["patterns"]), (other, w)
            assert (tmp_path / f"{other}.{w}.kmv.tsv").read_bytes() == (tmp_path / f"pv.{w}.kmv.tsv").read_bytes(), (other, w)
            with np.load(str(tmp_path / f"{other}.{w}.kma")) as a, np.load(f"{proj}.{w}.kma") as b:
                assert a["matrix"].tobytes() == b["matrix"].tobytes(), (other, w)

    run_py("extract.py", str(tmp_path / "x"), "--present", kins[2], kins[7], "--absent", kins[4], cwd=str(tmp_path), env=env)
    selected = json.load(open(tmp_path / "x.kmx.json"))["n_selected"]
    assert selected == patterns.count_where(first["001-255"]["patterns"], N, all_of=[2, 7], none_of=[4]) > 0
