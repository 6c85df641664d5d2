"""GPU: k_occgram (pk_occgram_device_accumulate) against numpy on mixed and adversarial tables, its accumulation over
sub-slices, the no-wrap case, the full-size N = 13 pass against float64 matmuls and a k_spectrum pass, and the
`merger.py --kwip` command line."""

import numpy as np
import pytest

from pykmer_amd import kwip, merger, spectrum
from gpu_support import env_without_ranks, family_kins, run_py
from merge_ref import direct_kernel, numpy_occgram

pytestmark = pytest.mark.gpu


def _device_occgram(gpu, tabs, cuts=None):
    N, n = len(tabs), tabs[0].size
    bufs = [gpu.DeviceBuffer(max(16, n)) for _ in tabs]
    acc = gpu.DeviceBuffer(gpu.occgram_words(N) * 8)
    try:
        for b, t in zip(bufs, tabs):
            b.upload(t)
        acc.zero()
        for a, b in (cuts or [(0, n)]):
            gpu.occgram_device_accumulate([buf.ptr + a for buf in bufs], b - a, acc.ptr)
        return acc.download().view(np.uint64).copy()
    finally:
        for b in bufs + [acc]:
            b.free()


def _mixed(rng, N, n):
    """Related tables: a shared core, per-table gains and losses, dense and sparse stretches, counts 1..255."""
    core = rng.random(n) < np.where(np.arange(n) < n // 3, 0.9, 0.1)
    out = []
    for i in range(N):
        keep = core ^ (rng.random(n) < 0.02 + 0.1 * (i % 3) / 3)
        small = rng.integers(1, 4, n)
        big = rng.integers(1, 256, n)
        out.append((np.where(rng.random(n) < 0.2, big, small) * keep).astype(np.uint8))
    return out


@pytest.mark.parametrize("N", [2, 3, 8, 13, 16, 17, 24, 32, 64, 128])
def test_occgram_vs_numpy(gpu, N):
    rng = np.random.default_rng(N)
    for n in ((1, 1000, 3 * 8192 + 1037, 4 ** 8 + 11) if N <= 32 else (1037, 2 ** 15 + 11)):
        tabs = _mixed(rng, N, n)
        assert np.array_equal(_device_occgram(gpu, tabs), numpy_occgram(tabs)), (N, n)


@pytest.mark.parametrize("N", [5, 20])
def test_occgram_adversarial(gpu, N):
    n = 70_001
    rng = np.random.default_rng(3)
    cases = {
        "zero": [np.zeros(n, np.uint8) for _ in range(N)],
        "255": [np.full(n, 255, np.uint8) for _ in range(N)],
        "one_table": [rng.integers(0, 256, n).astype(np.uint8)] + [np.zeros(n, np.uint8) for _ in range(N - 1)],
        "identical": [rng.integers(0, 256, n).astype(np.uint8)] * N,
    }
    side = []
    for i in range(N):
        t = np.zeros(n, np.uint8)
        t[: n // 2] = rng.integers(1, 256, n // 2)                               # dense
        sparse = rng.random(n - n // 2) < 0.01 * (i + 1) / N
        t[n // 2:] = rng.integers(1, 256, n - n // 2) * sparse                   # sparse, beside it
        side.append(t)
    cases["dense_sparse"] = side
    for name, tabs in cases.items():
        got = _device_occgram(gpu, tabs)
        assert np.array_equal(got, numpy_occgram(tabs)), name
        occ_hist, lin, gram = kwip.split_accumulator(got, N)
        if name == "255":
            assert int(occ_hist[N]) == n and not occ_hist[:N].any() and not gram[:N - 1].any()
        if name == "one_table":
            assert not occ_hist[2:].any() and not gram[1:].any()


def test_occgram_accumulates_over_sub_slices_and_repeats(gpu):
    rng = np.random.default_rng(11)
    n = 300_001
    for N in (7, 19):
        tabs = _mixed(rng, N, n)
        one = _device_occgram(gpu, tabs)
        assert np.array_equal(one, numpy_occgram(tabs))
        cuts = [(0, 2048), (2048, 100_352), (100_352, 100_368), (100_368, n)]
        assert np.array_equal(_device_occgram(gpu, tabs, cuts), one)
        assert np.array_equal(_device_occgram(gpu, tabs), one)                   # bit-identical on repeat


def test_occgram_refusals(gpu):
    buf = gpu.DeviceBuffer(4096)
    try:
        for N in (1, 129):
            with pytest.raises(ValueError, match="2 to 128"):
                gpu.occgram_device_accumulate([buf.ptr] * N, 64, buf.ptr)
        with pytest.raises(ValueError, match="16-byte aligned"):
            gpu.occgram_device_accumulate([buf.ptr, buf.ptr + 8], 64, buf.ptr)
        with pytest.raises(ValueError, match="null accumulator"):
            gpu.occgram_device_accumulate([buf.ptr, buf.ptr], 64, 0)
    finally:
        buf.free()


def test_occgram_counters_do_not_wrap(gpu):
    """Two all-255 tables of 2^32 + 4096 bytes: one class, every address a 65025 product, past 2^32 addresses."""
    import torch
    torch.cuda.empty_cache()
    n = 2 ** 32 + 4096
    a = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    b = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    acc = torch.zeros(gpu.occgram_words(2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu.occgram_device_accumulate([a.data_ptr(), b.data_ptr()], n, acc.data_ptr())
    occ_hist, lin, gram = kwip.split_accumulator(acc.cpu().numpy().view(np.uint64), 2)
    assert occ_hist.tolist() == [0, 0, n]
    assert gram[1].tolist() == [n * 65025] * 3 and not gram[0].any()
    assert lin[1].tolist() == [n * 255] * 2 and not lin[0].any()
    del a, b
    torch.cuda.empty_cache()


def test_occgram_full_size_n13(gpu):
    """4^15-byte genome-like tables resident in HBM (a shared core, per-table gains and losses, mostly small counts): every
    class's products against float64 matmuls over the class's addresses on the device (exact in chunks), the occupancy
    histogram against torch, and the unweighted sums against a k_spectrum pass of the same tables."""
    import torch
    torch.cuda.empty_cache()
    n, N = 4 ** 15, 13
    g = torch.Generator(device="cuda").manual_seed(13)
    core = torch.rand(n, device="cuda", generator=g) < 0.04
    tabs = []
    for i in range(N):
        flip = torch.rand(n, device="cuda", generator=g) < 0.002 * (1 + i % 4)
        small = torch.randint(1, 4, (n,), dtype=torch.uint8, device="cuda", generator=g)
        big = torch.randint(1, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
        t = torch.where(torch.rand(n, device="cuda", generator=g) < 0.02, big, small)
        tabs.append(t * (core ^ flip))
        del flip, small, big, t
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in tabs]
    acc = torch.zeros(gpu.occgram_words(N), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    secs = gpu.occgram_device_accumulate(ptrs, n, acc.data_ptr())
    occ_hist, lin, gram = kwip.split_accumulator(acc.cpu().numpy().view(np.uint64), N)

    want_g = np.zeros((N, N, N), dtype=np.int64)
    want_l = np.zeros((N, N), dtype=np.int64)
    want_h = np.zeros(N + 1, dtype=np.int64)
    chunk = 2 ** 26
    for lo in range(0, n, chunk):
        X = torch.stack([t[lo:lo + chunk] for t in tabs])
        occ = (X > 0).sum(dim=0)
        cnt = torch.bincount(occ, minlength=N + 1)
        want_h += cnt.cpu().numpy()
        on, order = torch.sort(occ)                                              # the addresses of each class, contiguous
        Xs = X[:, order[int(cnt[0]):]].to(torch.float64)
        start = 0
        for o in range(1, N + 1):
            Xm = Xs[:, start:start + int(cnt[o])]
            start += int(cnt[o])
            want_g[o - 1] += (Xm @ Xm.T).round().to(torch.int64).cpu().numpy()
            want_l[o - 1] += Xm.sum(dim=1).round().to(torch.int64).cpu().numpy()
        del X, occ, on, order, Xs, Xm
    iu = np.triu_indices(N)
    assert np.array_equal(occ_hist.astype(np.int64), want_h)
    assert np.array_equal(lin.astype(np.int64), want_l)
    for o in range(1, N + 1):
        assert np.array_equal(gram[o - 1].astype(np.int64), want_g[o - 1][iu]), o

    sacc = torch.zeros(gpu.spectrum_words(N), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu.spectrum_device_accumulate(ptrs, n, sacc.data_ptr())
    hist, joint = spectrum.expand_accumulator(sacc.cpu().numpy().view(np.uint64), N, n)
    ab = np.outer(np.arange(256), np.arange(256)).astype(np.uint64)
    total = gram.sum(axis=0, dtype=np.uint64)
    pairs = [tuple(p) for p in kwip.pair_list(N)]
    for p, (i, j) in enumerate(spectrum.pair_list(N)):
        assert int(total[pairs.index((i, j))]) == int((joint[p] * ab).sum(dtype=np.uint64)), (i, j)
    for i in range(N):
        assert int(lin[:, i].sum()) == int((hist[i] * np.arange(256, dtype=np.uint64)).sum())
    print(f"occgram N=13 k=15 kernel {secs * 1e3:.3f} ms")


def test_kwip_command_lines(gpu, tmp_path, manifest, monkeypatch):
    """indexer.py -> merger.py --kwip on the G7 FASTA inputs: the .kmo equals numpy over the tables, the .kern the direct
    restatement; the same files from .kin.bgz inputs in forced sub-slices and from two ranks (gloo on the one GPU)."""
    import gzip
    kins = family_kins(tmp_path, manifest)
    env = env_without_ranks()
    proj = str(tmp_path / "kw")
    r = run_py("merger.py", proj, *kins, "--kwip", cwd=str(tmp_path), env=env)
    assert r.stdout.count("saving") == 4 and not list(tmp_path.glob("kw*.kma"))
    tabs = [merger.Header(k, index_file=k).read_table_slice(0, 4 ** 7) for k in sorted(kins)]
    occ = kwip.load(proj + ".kmo")
    for key, w in zip(("occ_hist", "lin", "gram"), kwip.split_accumulator(numpy_occgram(tabs), len(tabs))):
        assert np.array_equal(occ[key], w), key
    k = np.loadtxt(proj + ".kern", skiprows=1, usecols=range(1, len(tabs) + 1))
    assert np.allclose(k, direct_kernel(tabs), rtol=1e-12, atol=0)

    bgz = []
    for kin in kins:
        with open(kin, "rb") as fh, gzip.open(kin + ".bgz", "wb") as out:
            out.write(fh.read())
        bgz.append(kin + ".bgz")
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(13 * 4096))
    merger.merge(str(tmp_path / "sub"), sorted(bgz), kwip=True)
    monkeypatch.delenv("PK_MERGE_HBM_BUDGET")
    assert (tmp_path / "sub.kern").read_bytes() == (tmp_path / "kw.kern").read_bytes()

    run_py("merger.py", str(tmp_path / "two"), *kins, "--kwip", "--gpus", "2", cwd=str(tmp_path),
         env=dict(env, PK_DIST_BACKEND="gloo"))
    for ext in ("kern", "dist"):
        assert (tmp_path / f"two.{ext}").read_bytes() == (tmp_path / f"kw.{ext}").read_bytes()
    two = kwip.load(str(tmp_path / "two.kmo"))
    assert np.array_equal(two["gram"], occ["gram"]) and np.array_equal(two["occ_hist"], occ["occ_hist"])
