"""CPU: kWIP's entropy-weighted kernel and distance on the host side -- the accumulator layout, weights, kernel and distance
against a direct per-address restatement, the .kmo format and its invariants, `merge(kwip=True)` on the G7 inputs, the
cross-check against the joint spectra, the CLI flag and its refusals, the gloo-sharded path, `python -m pykmer_amd.kwip`
and the tree.  The slice accumulators come from numpy here (no GPU in this suite); on GPUs the same code path calls
pk_occgram_device_accumulate."""
import json
import os

import numpy as np
import pytest

from gpu_support import run_py
from host_support import family_indexes, gloo_merge
from merge_ref import direct_kernel, numpy_occgram, numpy_occgram_partial, numpy_spectrum_partial
from pykmer_amd import _lib, kwip, merger, spectrum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tables(rng, N, n):
    shared = rng.random(n) < 0.3
    out = []
    for i in range(N):
        keep = shared ^ (rng.random(n) < 0.05 + 0.02 * (i % 4))
        out.append((rng.integers(1, 256, n) * keep).astype(np.uint8))
    return out


def test_occgram_words_and_pair_order():
    assert _lib.occgram_words(13) == 14 + 169 + 13 * 91
    assert kwip.pair_list(3).tolist() == [[0, 0], [0, 1], [0, 2], [1, 1], [1, 2], [2, 2]]
    assert kwip.pair_list(2).dtype == np.int32
    acc = np.arange(_lib.occgram_words(4), dtype=np.uint64)
    occ_hist, lin, gram = kwip.split_accumulator(acc, 4)
    assert occ_hist.tolist() == [0, 1, 2, 3, 4] and lin.shape == (4, 4) and int(lin[0, 0]) == 5
    assert gram.shape == (4, 10) and int(gram[0, 0]) == 21 and int(gram[-1, -1]) == acc.size - 1


@pytest.mark.parametrize("N", [2, 3, 7, 13, 32])
def test_weights(N):
    w = kwip.weights(N)
    assert w[0] == 0 and w[N] == 0 and np.all(w[1:N] > 0) and np.all(w <= 1)
    assert np.array_equal(w, w[::-1])
    if N % 2 == 0:
        assert w[N // 2] == 1.0
    assert np.array_equal(kwip.weights(N, unweighted=True), np.ones(N + 1))


@pytest.mark.parametrize("N", [2, 5, 13])
@pytest.mark.parametrize("unweighted", [False, True])
def test_kernel_and_distance_match_direct_restatement(N, unweighted):
    rng = np.random.default_rng(N)
    tabs = _tables(rng, N, 4 ** 6 + 5)
    _, lin, gram = kwip.split_accumulator(numpy_occgram(tabs), N)
    for i, t in enumerate(tabs):
        assert int(lin[:, i].sum()) == int(t.sum(dtype=np.uint64))          # sum_o lin[o][i] is the table's sum
    k = kwip.kernel(lin, gram, kwip.weights(N, unweighted))
    want = direct_kernel(tabs, unweighted)
    assert np.allclose(k, want, rtol=1e-12, atol=0)
    d = kwip.distance(k)
    dk = np.sqrt(np.maximum(0, 2 - 2 * want / np.sqrt(np.outer(np.diag(want), np.diag(want)))))
    np.fill_diagonal(dk, 0)
    assert np.allclose(d, dk, rtol=1e-12, atol=1e-12) and np.array_equal(d, d.T)


def test_distance_of_empty_sample_is_nan(capsys):
    # table 2 holds only k-mers every sample holds: weight 0, K(2, 2) = 0
    t0 = np.array([1, 2, 0, 5], np.uint8)
    t1 = np.array([3, 0, 4, 1], np.uint8)
    t2 = np.array([0, 0, 0, 7], np.uint8)
    _, lin, gram = kwip.split_accumulator(numpy_occgram([t0, t1, t2]), 3)
    k = kwip.kernel(lin, gram, kwip.weights(3))
    assert k[2, 2] == 0
    d = kwip.distance(k, ["a", "b", "c"])
    assert np.isnan(d[2]).all() and np.isnan(d[:, 2]).all() and np.isfinite(d[:2, :2]).all()
    assert "sample c" in capsys.readouterr().err


def test_library_refuses_bad_calls():
    for N in (0, 1, 129):
        with pytest.raises(ValueError, match="2 to 128 tables"):
            _lib.occgram_device_accumulate([4096] * N, 64, 4096)
    with pytest.raises(ValueError, match="null accumulator"):
        _lib.occgram_device_accumulate([4096] * 2, 64, 0)
    with pytest.raises(ValueError, match="16-byte aligned"):
        _lib.occgram_device_accumulate([4096, 4104], 64, 4096)


def _family(tmp_path, manifest, n=13):
    return sorted(family_indexes(tmp_path, manifest, n=n))


def test_merge_writes_kmo_kern_dist(tmp_path, manifest, monkeypatch):
    paths = _family(tmp_path, manifest)
    N = len(paths)
    calls = []

    def partial(*a):
        calls.append(a[1:3])
        return numpy_occgram_partial(*a)
    monkeypatch.chdir(tmp_path)
    data, k = merger.merge("kw", paths, partial_fn=partial, devices=(0, 1), kwip=True)
    assert sorted(calls) == [(0, 4 ** 7 // 2), (4 ** 7 // 2, 4 ** 7)]
    assert not list(tmp_path.glob("kw*.kma*"))                                  # no .kma
    tabs = [merger.Header(p, index_file=p).read_table_slice(0, 4 ** 7) for p in paths]
    occ = kwip.load("kw.kmo")
    want = kwip.split_accumulator(numpy_occgram(tabs), N)
    for key, w in zip(("occ_hist", "lin", "gram"), want):
        assert occ[key].dtype == np.uint64 and np.array_equal(occ[key], w), key
    assert occ["pairs"].tolist() == kwip.pair_list(N).tolist() and occ["kmer_len"] == 7 and occ["data_size"] == 4 ** 7
    with np.load("kw.kmo") as z:
        assert sorted(z.keys()) == ["data_size", "gram", "kmer_len", "lin", "occ_hist", "pairs"]
    meta = json.load(open("kw.kmo.json"))
    assert sorted(meta.keys()) == ["data", "data_size", "kmer_len", "project_name"] and meta["project_name"] == "kw"
    ids = [d["header"]["input_file_name"] for d in meta["data"]]
    assert ids == [os.path.basename(p)[: -len(".07.kin")] for p in paths]             # the FASTA each table was counted from
    assert np.allclose(k, direct_kernel(tabs), rtol=1e-12, atol=0)
    for name, m in (("kw.kern", k), ("kw.dist", kwip.distance(k))):
        lines = open(name).read().splitlines()
        assert lines[0] == "\t" + "\t".join(ids) and len(lines) == N + 1
        for line, row, sample in zip(lines[1:], m, ids):
            cols = line.split("\t")
            assert cols[0] == sample and [float(c) for c in cols[1:]] == row.tolist()
    d = np.loadtxt("kw.dist", skiprows=1, usecols=range(1, N + 1))
    assert np.all(np.diag(d) == 0) and np.all(d[~np.eye(N, dtype=bool)] > 0)
    # the tables deleted, the .kmo writes both matrices again, byte for byte
    for p in paths:
        os.remove(p)
    env = dict(os.environ, PYTHONPATH=ROOT)
    run_py("-m", "pykmer_amd.kwip", "kw.kmo", "--kernel", "again.kern", "--distance", "again.dist", cwd=str(tmp_path), env=env)
    assert (tmp_path / "again.kern").read_bytes() == (tmp_path / "kw.kern").read_bytes()
    assert (tmp_path / "again.dist").read_bytes() == (tmp_path / "kw.dist").read_bytes()
    kwip.main(["kw.kmo", "--kernel", "flat.kern", "--unweighted"])
    assert np.allclose(np.loadtxt("flat.kern", skiprows=1, usecols=range(1, N + 1)), direct_kernel(tabs, unweighted=True), rtol=1e-12)
    with pytest.raises(SystemExit):                                              # refuses to overwrite
        kwip.main(["kw.kmo", "--kernel", "flat.kern"])
    with pytest.raises(AssertionError, match="already exists"):
        merger.merge("kw", paths, partial_fn=numpy_occgram_partial, kwip=True)


def test_unweighted_sums_match_spectrum(tmp_path, manifest):
    """sum_o lin[o][i] is table i's sum, and the unweighted cross products sum_o G[o][i][j] equal sum a b J_ij[a][b] of the
    joint spectra the merger writes for the same tables."""
    paths = _family(tmp_path, manifest, n=6)
    merger.merge(str(tmp_path / "s"), paths, spectrum=True, partial_fn=numpy_spectrum_partial)
    merger.merge(str(tmp_path / "k"), paths, kwip=True, partial_fn=numpy_occgram_partial)
    spec, occ = spectrum.load(tmp_path / "s.kms"), kwip.load(tmp_path / "k.kmo")
    ab = np.outer(np.arange(256), np.arange(256)).astype(np.uint64)
    total = occ["gram"].sum(axis=0, dtype=np.uint64)
    pairs = [tuple(p) for p in kwip.pair_list(6)]
    for p, (i, j) in enumerate(spectrum.pair_list(6)):
        assert int(total[pairs.index((i, j))]) == int((spec["joint"][p] * ab).sum(dtype=np.uint64)), (i, j)
    for i in range(6):
        assert int(occ["lin"][:, i].sum()) == int((spec["hist"][i] * np.arange(256, dtype=np.uint64)).sum())
    assert int(occ["occ_hist"][1:].sum()) == int(np.count_nonzero(np.stack(
        [merger.Header(p, index_file=p).read_table_slice(0, 4 ** 7) for p in paths]).any(axis=0)))


def test_kmo_load_refuses_broken_invariants(tmp_path):
    tabs = _tables(np.random.default_rng(4), 4, 5000)
    occ_hist, lin, gram = (x.copy() for x in kwip.split_accumulator(numpy_occgram(tabs), 4))
    kwip.save(str(tmp_path / "ok"), occ_hist, lin, gram, 6, 5000, [])
    assert np.array_equal(kwip.load(tmp_path / "ok.kmo")["gram"], gram)
    with pytest.raises(AssertionError, match="already exists"):
        kwip.save(str(tmp_path / "ok"), occ_hist, lin, gram, 6, 5000, [])

    def broken(name, **kw):
        a = {"occ_hist": occ_hist.copy(), "lin": lin.copy(), "gram": gram.copy()}
        for key, (idx, val) in kw.items():
            a[key][idx] = val
        kwip.save(str(tmp_path / name), a["occ_hist"], a["lin"], a["gram"], 6, 5000, [])
        return tmp_path / f"{name}.kmo"
    with pytest.raises(AssertionError, match="data_size"):
        kwip.load(broken("h", occ_hist=(0, int(occ_hist[0]) + 1)))
    with pytest.raises(AssertionError, match="class 1"):
        kwip.load(broken("c", gram=((0, 1), 3)))
    z = np.flatnonzero(lin[1] == 0)
    assert not len(z)
    with pytest.raises(AssertionError, match="lin and the gram diagonal"):
        kwip.load(broken("l", lin=((1, 2), 0)))


def test_merger_cli_kwip_flag_and_refusals(tmp_path, capsys):
    args = merger.build_parser().parse_args(["p", "a.kin", "b.kin", "--kwip"])
    assert args.kwip and not merger.build_parser().parse_args(["p", "a.kin", "b.kin"]).kwip
    for extra in (["--spectrum"], ["--sweep", "1-3"], ["--min-count", "2"], ["--max-count", "50"]):
        with pytest.raises(SystemExit) as e:
            merger.main(["p", str(tmp_path / "a.kin"), str(tmp_path / "b.kin"), "--kwip"] + extra)
        assert e.value.code == 2
        assert "--kwip takes no" in capsys.readouterr().err
    with pytest.raises(AssertionError):
        merger.merge("p", [tmp_path / "a.kin"], kwip=True, windows=[(1, 3)])


def test_calculate_distance_builds_the_kwip_tree(tmp_path, manifest):
    paths = _family(tmp_path, manifest, n=5)
    proj = str(tmp_path / "tree")
    merger.merge(proj, paths, kwip=True, partial_fn=numpy_occgram_partial)
    run_py("calculate_distance.py", proj + ".kmo", cwd=str(tmp_path))
    base = proj + ".kmo.dist.kwip"
    d = np.load(base + ".mat.redundant.np")
    assert np.array_equal(d, kwip.matrices(kwip.load(proj + ".kmo"))[1])
    assert np.array_equal(np.load(base + ".npz")["distance"], d)
    newick = open(base + ".newick").read()
    ids = [os.path.basename(p)[: -len(".07.kin")] for p in paths]
    for i in ids:
        assert i in newick
    assert open(base + ".mat.redundant.lsmat").readline().rstrip("\n").split("\t")[1:] == ids
    assert np.allclose(np.loadtxt(base + ".mat.condensed.txt"), d[np.triu_indices(5, 1)])


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_kwip_matches_single_process(tmp_path, manifest, world):
    paths = _family(tmp_path, manifest)
    gloo_merge(world, tmp_path, paths, numpy_occgram_partial, kwip=True)
    merger.merge(str(tmp_path / "one"), paths, kwip=True, partial_fn=numpy_occgram_partial)
    one, dist_ = kwip.load(tmp_path / "one.kmo"), kwip.load(tmp_path / "dist.kmo")
    for key in ("occ_hist", "lin", "gram"):
        assert np.array_equal(one[key], dist_[key]), key
    assert (tmp_path / "one.kern").read_bytes() == (tmp_path / "dist.kern").read_bytes()
    assert (tmp_path / "one.dist").read_bytes() == (tmp_path / "dist.dist").read_bytes()
    slices = []
    for r in range(world):
        seen = np.load(tmp_path / f"slice_rank{r}.npy")
        assert len(seen) == 1
        lo, hi, delivered = (int(v) for v in seen[0])
        slices.append((lo, hi))
        assert delivered == len(paths) * (hi - lo) <= len(paths) * (4 ** 7 // world + 32)
    assert slices[0][0] == 0 and slices[-1][1] == 4 ** 7
    assert all(a[1] == b[0] for a, b in zip(slices[:-1], slices[1:]))
