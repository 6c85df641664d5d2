"""GPU: k_spectrum (pk_spectrum_device_accumulate) against numpy bincount on adversarial and genome-like tables, its
accumulation over sub-slices, the full-size N = 13 pass against the single-window scans, the no-wrap case, and the
`merger.py --spectrum` / `python -m pykmer_amd.spectrum` command lines."""
import json
import os

import numpy as np
import pytest

from pykmer_amd import merger, spectrum
from gpu_support import ROOT, env_without_ranks, family_kins, run_py
from merge_ref import device_bincount, numpy_spectrum

pytestmark = pytest.mark.gpu


def _device_spectrum(gpu, tabs, cuts=None):
    N, n = len(tabs), tabs[0].size
    bufs = [gpu.DeviceBuffer(max(16, n)) for _ in tabs]
    acc = gpu.DeviceBuffer(gpu.spectrum_words(N) * 8)
    try:
        for b, t in zip(bufs, tabs):
            b.upload(t)
        acc.zero()
        for a, b in (cuts or [(0, n)]):
            gpu.spectrum_device_accumulate([buf.ptr + a for buf in bufs], b - a, acc.ptr)
        return acc.download().view(np.uint64).copy()
    finally:
        for b in bufs + [acc]:
            b.free()


_GENOME = {}


def _genome_table(gpu, i, n):
    """Member i of the synthetic family counted at k = 9 by the indexer, cut or repeated to n bytes."""
    if i not in _GENOME:
        import synth
        fa, _ = synth.family(i, 60_000)
        _GENOME[i] = gpu.count_fasta(fa, 9)["table"]
    t = _GENOME[i]
    return np.resize(t, n).astype(np.uint8)


def _table(gpu, kind, rng, n, i):
    if kind == "genome":
        return _genome_table(gpu, i % 5, n)
    if kind == "ones":
        return np.ones(n, np.uint8)
    if kind == "255":
        return np.full(n, 255, np.uint8)
    if kind == "zero":
        return np.zeros(n, np.uint8)
    keep = rng.random(n) < 0.4
    if kind == "uniform":
        return (rng.integers(1, 256, n) * keep).astype(np.uint8)
    return (np.minimum(rng.poisson(30, n), 255) * keep).astype(np.uint8)   # coverage-like


KINDS = ["genome", "ones", "255", "uniform", "poisson", "zero"]


@pytest.mark.parametrize("N", [2, 3, 8, 13, 17, 32])
def test_spectrum_vs_bincount(gpu, N):
    rng = np.random.default_rng(N)
    for n in (1, 31, 2047, 4 ** 7, 4 ** 9 + 17):
        for shift in range(2 if N <= 3 else 1):        # N = 2, 3: every distribution meets every other
            tabs = [_table(gpu, KINDS[(i + shift * 3 + n) % len(KINDS)], rng, n, i) for i in range(N)]
            got = _device_spectrum(gpu, tabs)
            want = numpy_spectrum(tabs)
            assert np.array_equal(got, want), (N, n, shift)


@pytest.mark.parametrize("kind", ["ones", "255", "uniform", "poisson", "genome"])
def test_spectrum_single_distribution(gpu, kind):
    """Every table of one distribution: a single hot bin ((1,1), (255,255)), every bin, coverage depth, genome counts."""
    rng = np.random.default_rng(5)
    tabs = [_table(gpu, kind, rng, 4 ** 9 + 17, i) for i in range(5)]
    assert np.array_equal(_device_spectrum(gpu, tabs), numpy_spectrum(tabs))


def test_spectrum_accumulates_over_sub_slices_and_repeats(gpu):
    rng = np.random.default_rng(11)
    n = 300_001
    tabs = [_table(gpu, KINDS[i % len(KINDS)], rng, n, i) for i in range(7)]
    one = _device_spectrum(gpu, tabs)
    assert np.array_equal(one, numpy_spectrum(tabs))
    cuts = [(0, 2048), (2048, 100_352), (100_352, 100_368), (100_368, n)]
    assert np.array_equal(_device_spectrum(gpu, tabs, cuts), one)
    assert np.array_equal(_device_spectrum(gpu, tabs), one)                   # bit-identical on repeat


def test_spectrum_refuses_more_than_128_tables(gpu):
    buf = gpu.DeviceBuffer(4096)
    try:
        with pytest.raises(ValueError, match="2 to 128"):
            gpu.spectrum_device_accumulate([buf.ptr] * 129, 64, buf.ptr)
    finally:
        buf.free()


def test_spectrum_full_size_n13(gpu):
    """4^15-byte tables resident in HBM: histograms against pk_table_stats and torch, the marginal invariants, 16 windows
    against pk_gram_device_accumulate_windows (every entry) and four pairs against torch.bincount on the device."""
    import torch
    torch.cuda.empty_cache()
    n, N = 4 ** 15, 13
    g = torch.Generator(device="cuda").manual_seed(13)
    tabs = []
    for i in range(N):
        small = torch.randint(1, 4, (n,), dtype=torch.uint8, device="cuda", generator=g)
        big = torch.randint(1, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
        t = torch.where(torch.rand(n, device="cuda", generator=g) < 0.02, big, small)
        tabs.append(t * (torch.rand(n, device="cuda", generator=g) < 0.04 + 0.03 * i))
        del small, big
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in tabs]
    acc = torch.zeros(gpu.spectrum_words(N), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    secs = gpu.spectrum_device_accumulate(ptrs, n, acc.data_ptr())
    hist, joint = spectrum.expand_accumulator(acc.cpu().numpy().view(np.uint64), N, n)
    for i in (0, 12):
        assert np.array_equal(hist[i], gpu.table_stats(tabs[i].cpu().numpy()))
    for i in range(N):
        assert np.array_equal(hist[i], device_bincount(tabs[i].to(torch.int32), 256)), i
    for p, (i, j) in enumerate(spectrum.pair_list(N)):
        assert int(joint[p].sum()) == n
        assert np.array_equal(joint[p].sum(axis=1), hist[i]) and np.array_equal(joint[p].sum(axis=0), hist[j])
    wins = [(1, 255), (2, 255), (1, 3), (2, 5), (1, 1), (255, 255), (3, 255), (1, 2),
            (128, 255), (100, 200), (1, 127), (129, 254), (2, 2), (3, 3), (4, 50), (1, 50)]
    dev = torch.zeros((len(wins), N, N), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu.gram_device_accumulate_windows(ptrs, n, dev.data_ptr(), wins)
    want = dev.cpu().numpy().view(np.uint64)
    for w, got in enumerate(spectrum.window_pairs(hist, joint, wins)):
        assert np.array_equal(got, want[w]), wins[w]
    for i, j in ((0, 1), (3, 11), (5, 12), (11, 12)):
        p = i * N - i * (i + 1) // 2 + (j - i - 1)
        b = device_bincount(tabs[i].to(torch.int32) * 256 + tabs[j].to(torch.int32), 65536)
        assert np.array_equal(joint[p], b.reshape(256, 256)), (i, j)
    print(f"spectrum N=13 k=15 kernel {secs * 1e3:.3f} ms")


def test_spectrum_counters_do_not_wrap(gpu):
    """Two all-ones tables of 2^32 + 4096 bytes: every address is a (1,1) event -- the single hot bin, past 2^32."""
    import torch
    torch.cuda.empty_cache()
    n = 2 ** 32 + 4096
    a = torch.ones(n, dtype=torch.uint8, device="cuda")
    b = torch.ones(n, dtype=torch.uint8, device="cuda")
    acc = torch.zeros(gpu.spectrum_words(2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu.spectrum_device_accumulate([a.data_ptr(), b.data_ptr()], n, acc.data_ptr())
    hist, core = spectrum.split_accumulator(acc.cpu().numpy().view(np.uint64), 2)
    assert int(core[0, 0, 0]) == n and int(core.sum()) == n
    assert [int(hist[i, 1]) for i in (0, 1)] == [n, n] and int(hist.sum()) == 2 * n
    del a, b
    torch.cuda.empty_cache()


def _same_kms(a, b):
    x, y = spectrum.load(a), spectrum.load(b)
    return np.array_equal(x["hist"], y["hist"]) and np.array_equal(x["joint"], y["joint"])


def test_spectrum_command_lines(gpu, tmp_path, manifest, monkeypatch):
    """merger.py --spectrum on the G7 family against the goldens; the same .kms from .kin.bgz inputs in forced sub-slices,
    from two ranks (gloo) and from ResidentTable inputs; the spectrum CLI re-derives the windows with the .kin files gone."""
    import gzip
    kins = family_kins(tmp_path, manifest)
    want = {tag: np.array(manifest["merger"][f"G7_k7_n13_{tag}"]["matrix"], dtype=np.uint64) for tag in ("min2", "max3", "default")}
    env = env_without_ranks()
    proj = str(tmp_path / "sp")
    r = run_py("merger.py", proj, *kins, "--spectrum", "--sweep", "2-255,1-3", cwd=str(tmp_path), env=env)
    assert r.stdout.count("saving") == 6
    assert np.array_equal(np.load(proj + ".002-255.kma")["matrix"], want["min2"])
    assert np.array_equal(np.load(proj + ".001-003.kma")["matrix"], want["max3"])

    # .kin.bgz inputs, sub-slices forced by the HBM budget
    bgz = []
    for k in kins:
        with open(k, "rb") as fh, gzip.open(k + ".bgz", "wb") as out:
            out.write(fh.read())
        bgz.append(k + ".bgz")
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(13 * 4096))
    merger.merge(str(tmp_path / "sub"), sorted(bgz), spectrum=True)
    monkeypatch.delenv("PK_MERGE_HBM_BUDGET")
    assert _same_kms(proj + ".kms", str(tmp_path / "sub.kms"))

    # two ranks on the one GPU (gloo: RCCL refuses two ranks on one device)
    r = run_py("merger.py", str(tmp_path / "two"), *kins, "--spectrum", "--gpus", "2", cwd=str(tmp_path),
             env=dict(env, PK_DIST_BACKEND="gloo"))
    assert _same_kms(proj + ".kms", str(tmp_path / "two.kms"))
    assert np.array_equal(np.load(str(tmp_path / "two.001-255.kma"))["matrix"], want["default"])

    # tables that never left HBM
    headers = [merger.Header(k, index_file=k) for k in sorted(kins)]
    tabs = [h.read_table_slice(0, h.data_size) for h in headers]
    bufs = [gpu.DeviceBuffer(t.size) for t in tabs]
    try:
        for b, t in zip(bufs, tabs):
            b.upload(t)
        res = [merger.ResidentTable(b.ptr, t.size, t.size, device=0) for b, t in zip(bufs, tabs)]
        total = merger.pair_spectrum(res)
    finally:
        for b in bufs:
            b.free()
    hist, joint = spectrum.expand_accumulator(total, len(tabs), 4 ** 7)
    ref = spectrum.load(proj + ".kms")
    assert np.array_equal(hist, ref["hist"]) and np.array_equal(joint, ref["joint"])

    # the windows again, from the .kms alone
    for k in kins + bgz:
        os.remove(k)
    (tmp_path / "d").mkdir()
    run_py("-m", "pykmer_amd.spectrum", proj + ".kms", "sp", "--sweep", "2-255,1-3", cwd=str(tmp_path / "d"),
         env=dict(env, PYTHONPATH=ROOT))
    for name, tag in (("sp.002-255.kma", "min2"), ("sp.001-003.kma", "max3")):
        assert np.array_equal(np.load(str(tmp_path / "d" / name))["matrix"], want[tag])
        meta = json.load(open(tmp_path / "d" / f"{name}.json"))
        direct = json.load(open(f"{proj}.{name[3:]}.json"))
        assert meta["data"] == direct["data"] and meta["project_name"] == "sp"
