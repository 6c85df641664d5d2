"""CPU: joint count spectra (.kms) on the host side -- windows derived from spectra against the oracle's pair tallies, the
reference goldens reproduced through `merge(spectrum=True)` and the spectrum CLI with the tables gone, the file format, and
the sharded (gloo) path.  The slice spectra come from numpy here (no GPU in this suite); on GPUs the same code path calls
pk_spectrum_device_accumulate."""
import json
import os

import numpy as np
import pytest

import oracle
from host_support import family_indexes, gloo_merge
from merge_ref import numpy_spectrum, numpy_spectrum_partial, oracle_partial
from pykmer_amd import _lib, merger, spectrum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = [(1, 255), (2, 255), (1, 3), (2, 5), (1, 1), (255, 255), (7, 3), (1, 50)]
GOLDEN_WINDOWS = [((1, 255), "default"), ((2, 255), "min2"), ((1, 3), "max3"), ((2, 5), "min2max5")]


def _tables(rng, N, n):
    out = []
    for i in range(N):
        t = rng.integers(1, 256, size=n, dtype=np.uint8)
        t[rng.random(n) > 0.3 + 0.05 * (i % 5)] = 0
        t[rng.random(n) < 0.1] = rng.integers(1, 6)           # plenty of small counts for the windows
        out.append(t)
    if N > 2:
        out[1][:] = 0                                          # an all-zero table
    return out


def test_spectrum_words_and_pair_order():
    assert _lib.spectrum_words(13) == 13 * 256 + 78 * 65025
    assert spectrum.pair_list(4).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert spectrum.pair_list(2).dtype == np.int32 and spectrum.pair_list(1).shape == (0, 2)


@pytest.mark.parametrize("N", [2, 5, 13])
def test_windows_from_spectra_match_oracle(N):
    rng = np.random.default_rng(N)
    n = 4 ** 6 + 5
    tabs = _tables(rng, N, n)
    hist, joint = spectrum.expand_accumulator(numpy_spectrum(tabs), N, n)
    for p, (i, j) in enumerate(spectrum.pair_list(N)):             # the expansion IS the full joint spectrum
        full = np.bincount(tabs[i].astype(np.int64) * 256 + tabs[j], minlength=65536).reshape(256, 256)
        assert np.array_equal(joint[p], full), (i, j)
    for (mn, mx), pair in zip(WINDOWS, spectrum.window_pairs(hist, joint, WINDOWS)):
        assert pair.dtype == np.uint64 and pair.shape == (N, N)
        assert np.array_equal(_lib.gram_expand(pair), oracle.gram(tabs, mn, mx)), (mn, mx)
        assert not np.tril(pair, -1).any()
        if mn > mx:
            assert not pair.any()


def test_expand_refuses_inconsistent_spectra():
    tabs = _tables(np.random.default_rng(3), 3, 1000)
    acc = numpy_spectrum(tabs)
    hist, core = spectrum.split_accumulator(acc.copy(), 3)
    core[0, 4, 4] += 10 ** 6
    with pytest.raises(AssertionError):
        spectrum.expand(hist, core, 1000)


def test_library_refuses_bad_table_counts():
    for N in (0, 1, 129):
        with pytest.raises(ValueError, match="2 to 128 tables"):
            _lib.spectrum_device_accumulate([4096] * N, 64, 4096)
    with pytest.raises(ValueError, match="null accumulator"):
        _lib.spectrum_device_accumulate([4096] * 2, 64, 0)


def _want(manifest, tag):
    return np.array(manifest["merger"][f"G7_k7_n13_{tag}"]["matrix"], dtype=np.uint64)


def test_spectrum_merge_and_cli_reproduce_reference_goldens(tmp_path, manifest, monkeypatch):
    """G7 k=7 N=13: ONE spectrum pass writes the .kms and all four windows' .kma; with every .kin deleted the spectrum CLI
    derives them again, and its .kma.json is byte-equal to what a direct merge under the same project name writes."""
    paths = sorted(family_indexes(tmp_path, manifest))
    wins = [w for w, _ in GOLDEN_WINDOWS]
    calls = []

    def partial(*a):
        calls.append(a[1:3])
        return numpy_spectrum_partial(*a)
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    (tmp_path / "c").mkdir()
    monkeypatch.chdir(tmp_path / "a")
    data, first = merger.merge("proj", paths, windows=wins, spectrum=True, partial_fn=partial, devices=(0, 1))
    assert sorted(calls) == [(0, 4 ** 7 // 2), (4 ** 7 // 2, 4 ** 7)]            # one pass per device slice, no second scan
    assert np.array_equal(first, _want(manifest, "default"))
    for (mn, mx), tag in GOLDEN_WINDOWS:
        assert np.array_equal(np.load(f"proj.{mn:03d}-{mx:03d}.kma")["matrix"], _want(manifest, tag)), tag
    monkeypatch.chdir(tmp_path / "c")
    merger.merge("Q", paths, windows=wins, partial_fn=oracle_partial)           # the direct merge, for its .kma.json
    for p in paths:
        os.remove(p)
    assert not any(os.path.exists(p) for p in paths)
    monkeypatch.chdir(tmp_path / "b")
    spectrum.main([str(tmp_path / "a" / "proj.kms"), "Q", "--sweep", "1-255,2-255,1-3,2-5"])
    case = manifest["merger"]["G7_k7_n13_min2max5"]
    for (mn, mx), tag in GOLDEN_WINDOWS:
        name = f"Q.{mn:03d}-{mx:03d}.kma"
        kma = np.load(name)
        assert list(kma.keys()) == ["matrix"] and kma["matrix"].dtype == np.uint64
        assert np.array_equal(kma["matrix"], _want(manifest, tag)), tag
        assert (tmp_path / "b" / f"{name}.json").read_bytes() == (tmp_path / "c" / f"{name}.json").read_bytes()
        meta = json.load(open(f"{name}.json"))
        assert sorted(meta.keys()) == case["kma_json_keys"]
        assert sorted(meta["data"][0].keys()) == case["kma_json_data0_keys"]
        assert sorted(meta["data"][0]["header"].keys()) == case["kma_json_header_keys"]
        assert [os.path.basename(d["index_file"]) for d in meta["data"]] == case["order"]
    spectrum.main([str(tmp_path / "a" / "proj.kms"), "R", "--min-count", "2", "--max-count", "5"])
    assert np.array_equal(np.load("R.002-005.kma")["matrix"], _want(manifest, "min2max5"))
    with pytest.raises(AssertionError):                                          # refuses to overwrite
        spectrum.main([str(tmp_path / "a" / "proj.kms"), "R", "--min-count", "2", "--max-count", "5"])


def test_kms_round_trip_and_invariants(tmp_path, manifest):
    paths = sorted(family_indexes(tmp_path, manifest, n=5))
    proj = str(tmp_path / "rt")
    merger.merge(proj, paths, spectrum=True, partial_fn=numpy_spectrum_partial)
    with np.load(proj + ".kms") as z:
        assert sorted(z.keys()) == ["data_size", "hist", "joint", "kmer_len", "pairs"]
        assert z["hist"].dtype == np.uint64 and z["hist"].shape == (5, 256)
        assert z["joint"].dtype == np.uint64 and z["joint"].shape == (10, 256, 256)
        assert z["pairs"].dtype == np.int32 and z["pairs"].tolist() == spectrum.pair_list(5).tolist()
        assert int(z["kmer_len"]) == 7 and int(z["data_size"]) == 4 ** 7
    spec = spectrum.load(proj + ".kms")
    hist, joint = spec["hist"], spec["joint"]
    for p, (i, j) in enumerate(spec["pairs"]):
        assert int(joint[p].sum()) == spec["data_size"]
        assert np.array_equal(joint[p].sum(axis=1), hist[i]) and np.array_equal(joint[p].sum(axis=0), hist[j])
    meta = spec["meta"]
    assert sorted(meta.keys()) == ["data", "data_size", "kmer_len", "project_name"]
    assert meta["project_name"] == proj and meta["kmer_len"] == 7 and meta["data_size"] == 4 ** 7
    kma_meta = json.load(open(proj + ".001-255.kma.json"))
    assert meta["data"] == kma_meta["data"]                                      # exactly what the .kma.json holds
    assert not os.path.exists(proj + ".kms.tmp") and not os.path.exists(proj + ".kms.json.tmp")
    with pytest.raises(AssertionError, match="already exists"):
        spectrum.save(proj, hist, joint, 7, 4 ** 7, meta["data"])
    os.remove(proj + ".001-255.kma")
    os.remove(proj + ".001-255.kma.json")
    with pytest.raises(AssertionError, match="already exists"):                  # merge refuses before scanning
        merger.merge(proj, paths, spectrum=True, partial_fn=numpy_spectrum_partial)


def test_merger_cli_takes_spectrum_flag():
    args = merger.build_parser().parse_args(["p", "a.kin", "b.kin", "--spectrum", "--sweep", "1-3"])
    assert args.spectrum and args.sweep == "1-3"
    assert not merger.build_parser().parse_args(["p", "a.kin", "b.kin"]).spectrum


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_spectrum_matches_single_process(tmp_path, manifest, world):
    paths = sorted(family_indexes(tmp_path, manifest))
    gloo_merge(world, tmp_path, paths, numpy_spectrum_partial, windows=[(2, 255), (1, 3)], spectrum=True)
    merger.merge(str(tmp_path / "one"), paths, windows=[(2, 255)], spectrum=True, partial_fn=numpy_spectrum_partial)
    one, dist_ = spectrum.load(tmp_path / "one.kms"), spectrum.load(tmp_path / "dist.kms")
    assert np.array_equal(one["hist"], dist_["hist"]) and np.array_equal(one["joint"], dist_["joint"])
    assert np.array_equal(np.load(tmp_path / "dist.002-255.kma")["matrix"], _want(manifest, "min2"))
    assert np.array_equal(np.load(tmp_path / "dist.001-003.kma")["matrix"], _want(manifest, "max3"))
    slices = []
    for r in range(world):
        seen = np.load(tmp_path / f"slice_rank{r}.npy")
        assert len(seen) == 1                                                    # one pass per rank
        lo, hi, delivered = (int(v) for v in seen[0])
        slices.append((lo, hi))
        assert delivered == len(paths) * (hi - lo) <= len(paths) * (4 ** 7 // world + 32)   # each rank read its slice only
    assert slices[0][0] == 0 and slices[-1][1] == 4 ** 7
    assert all(a[1] == b[0] for a, b in zip(slices[:-1], slices[1:]))
