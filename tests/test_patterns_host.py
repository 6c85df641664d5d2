"""CPU: presence patterns on the host side -- the three derivations (pair matrix, occupancy, count_where) against direct
restatements, `merge(patterns=True)` on the G7 inputs with numpy as the slice pass (single process and gloo-sharded), the
.kmv / .kmv.json / .kmv.tsv formats, `python -m pykmer_amd.patterns` and the refusals.  On GPUs the same code path calls
pk_patterns_device_accumulate."""
import json
import os

import numpy as np
import pytest

from gpu_support import HostTable, run_py
from host_support import family_indexes, gloo_merge
from merge_ref import oracle_partial
from patterns_ref import bit_words, numpy_patterns, numpy_patterns_partial
from pykmer_amd import _lib, merger, patterns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = [(1, 255), (2, 255), (1, 1), (3, 50)]


def _tables(rng, N, n):
    shared = rng.random(n) < 0.3
    out = []
    for i in range(N):
        keep = shared ^ (rng.random(n) < 0.05 + 0.03 * (i % 5))
        vals = np.where(rng.random(n) < 0.5, rng.integers(1, 5, n), rng.integers(1, 256, n))
        out.append((vals * keep).astype(np.uint8))
    return out


def test_patterns_words():
    assert [_lib.patterns_words(N) for N in (1, 2, 13, 16)] == [2, 4, 8192, 65536]
    assert "pk_patterns_device_accumulate" in _lib.EXPORTS


@pytest.mark.parametrize("N", [1, 2, 5, 9, 16])
def test_identities(N):
    rng = np.random.default_rng(100 + N)
    n = 4 ** 5
    tabs = _tables(rng, N, n)
    headers = [HostTable(5, f"t{i}", t) for i, t in enumerate(tabs)]
    for (mn, mx), want_pair in zip(WINDOWS, oracle_partial(headers, 0, n, WINDOWS, 0, 1)):
        p = numpy_patterns(tabs, mn, mx)
        assert p.dtype == np.uint64 and p.shape == (1 << N,) and int(p.sum()) == n
        m = patterns.matrix_from_patterns(p, N)
        assert m.dtype == np.uint64 and m.shape == (N, N) and np.array_equal(m, want_pair), (N, mn, mx)
        words = bit_words(tabs, mn, mx)
        held = np.array([bin(int(w)).count("1") for w in words])
        occ = patterns.occupancy_from_patterns(p, N)
        assert occ.dtype == np.uint64 and np.array_equal(occ, np.bincount(held, minlength=N + 1)), (N, mn, mx)
        assert patterns.count_where(p, N) == n
        assert patterns.count_where(p, N, all_of=range(N)) == int(p[-1])
        for i in range(N):
            assert patterns.count_where(p, N, all_of=[i], none_of=[j for j in range(N) if j != i]) == int(p[1 << i])
        for _ in range(12):
            sets = [list(rng.choice(N, size=rng.integers(0, min(N, 3) + 1), replace=False)) for _ in range(3)]
            brute = 0
            for w in words:
                w = int(w)
                ok = all((w >> t) & 1 for t in sets[0]) and not any((w >> t) & 1 for t in sets[1])
                brute += ok and (not sets[2] or any((w >> t) & 1 for t in sets[2]))
            assert patterns.count_where(p, N, all_of=sets[0], none_of=sets[1], any_of=sets[2]) == brute, (N, mn, mx, sets)


def test_derivations_refuse_bad_arguments():
    p = np.zeros(8, np.uint64)
    with pytest.raises(ValueError, match="1 to 16 tables"):
        patterns.matrix_from_patterns(np.zeros(1 << 17, np.uint64), 17)
    with pytest.raises(AssertionError, match="8 patterns"):
        patterns.occupancy_from_patterns(p[:4], 3)
    with pytest.raises(ValueError, match="table 3"):
        patterns.count_where(p, 3, all_of=[3])


def _family(tmp_path, manifest, n=13):
    return sorted(family_indexes(tmp_path, manifest, n=n))


def _read(paths):
    return [merger.Header(p, index_file=p).read_table_slice(0, 4 ** 7) for p in paths]


def test_merge_writes_kmv_json_tsv_and_kma(tmp_path, manifest, monkeypatch):
    paths = _family(tmp_path, manifest)
    N = len(paths)
    monkeypatch.chdir(tmp_path)
    sweep = [(1, 255), (2, 255)]
    calls = []

    def partial(*a):
        calls.append(a[1:3])
        return numpy_patterns_partial(*a)
    merger.merge("pv", paths, partial_fn=partial, devices=(0, 1), windows=sweep, patterns=True)
    assert sorted(calls) == [(0, 4 ** 7 // 2), (4 ** 7 // 2, 4 ** 7)]
    merger.merge("plain", paths, partial_fn=oracle_partial, windows=sweep)
    assert sorted(f.name for f in tmp_path.glob("pv.*")) == sorted(
        f"pv.{w}.{ext}" for w in ("001-255", "002-255") for ext in ("kma", "kma.json", "kmv", "kmv.json", "kmv.tsv"))
    tabs = _read(paths)
    for mn, mx in sweep:
        stem = f"pv.{mn:03d}-{mx:03d}"
        assert [str(f) for f in patterns.pattern_paths("pv", mn, mx)] == [stem + e for e in (".kmv", ".kmv.json", ".kmv.tsv")]
        want = numpy_patterns(tabs, mn, mx)
        with np.load(stem + ".kmv") as z:
            assert sorted(z.keys()) == ["data_size", "kmer_len", "max_count", "min_count", "n_tables", "patterns"]
            assert z["patterns"].dtype == np.uint64 and np.array_equal(z["patterns"], want)
        kmv = patterns.load(stem + ".kmv")
        assert (kmv["n_tables"], kmv["kmer_len"], kmv["data_size"], kmv["min_count"], kmv["max_count"]) == (N, 7, 4 ** 7, mn, mx)
        with np.load(stem + ".kma") as a, np.load(f"plain.{mn:03d}-{mx:03d}.kma") as b:
            assert a["matrix"].dtype == b["matrix"].dtype and np.array_equal(a["matrix"], b["matrix"])
        meta, kma_meta = json.load(open(stem + ".kmv.json")), json.load(open(stem + ".kma.json"))
        assert sorted(meta.keys()) == sorted(list(kma_meta.keys()) + ["kmer_len", "data_size", "n_tables", "n_patterns", "pan", "core", "private"])
        assert meta["data"] == kma_meta["data"] and (meta["min_count"], meta["max_count"]) == (mn, mx)
        assert meta["n_tables"] == N and meta["kmer_len"] == 7 and meta["data_size"] == 4 ** 7
        assert meta["n_patterns"] == int(np.count_nonzero(want[1:])) and meta["pan"] == 4 ** 7 - int(want[0])
        assert meta["core"] == int(want[-1]) and meta["private"] == [int(want[1 << i]) for i in range(N)]
        lines = open(stem + ".kmv.tsv").read().splitlines()
        names = [d["header"]["project_name"] for d in meta["data"]]
        assert lines[0].split("\t") == names + ["n_tables", "count"] and len(lines) == 1 + meta["n_patterns"]
        rows = [[int(c) for c in line.split("\t")] for line in lines[1:]]
        seen = []
        for r in rows:
            assert set(r[:N]) <= {0, 1} and r[N] == sum(r[:N])
            q = sum(b << t for t, b in enumerate(r[:N]))
            assert q != 0 and r[N + 1] == int(want[q]) > 0
            seen.append((-r[N + 1], q))
        assert seen == sorted(seen) and len(set(seen)) == len(seen)          # count descending, then pattern ascending
    assert int(numpy_patterns(tabs, 1, 255)[1:].max()) > 0
    with pytest.raises(AssertionError, match="already exists"):              # an existing .kmv alone stops the run
        os.remove("pv.001-255.kma")
        os.remove("pv.001-255.kma.json")
        os.remove("pv.001-255.kmv.json")
        os.remove("pv.001-255.kmv.tsv")
        merger.merge("pv", paths, partial_fn=numpy_patterns_partial, windows=[(1, 255)], patterns=True)
    assert not os.path.exists("pv.001-255.kma") and not os.path.exists("pv.001-255.kmv.tsv")


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_patterns_match_single_process(tmp_path, manifest, world):
    paths = _family(tmp_path, manifest)
    sweep = [(1, 255), (3, 50)]
    gloo_merge(world, tmp_path, paths, numpy_patterns_partial, windows=sweep, patterns=True)
    merger.merge(str(tmp_path / "one"), paths, partial_fn=numpy_patterns_partial, windows=sweep, patterns=True)
    for mn, mx in sweep:
        w = f"{mn:03d}-{mx:03d}"
        one, dist_ = patterns.load(tmp_path / f"one.{w}.kmv"), patterns.load(tmp_path / f"dist.{w}.kmv")
        assert np.array_equal(one["patterns"], dist_["patterns"]) and int(one["patterns"].sum()) == 4 ** 7
        assert (tmp_path / f"one.{w}.kmv.tsv").read_bytes() == (tmp_path / f"dist.{w}.kmv.tsv").read_bytes()
        with np.load(tmp_path / f"one.{w}.kma") as a, np.load(tmp_path / f"dist.{w}.kma") as b:
            assert np.array_equal(a["matrix"], b["matrix"])
    slices = []
    for r in range(world):
        seen = np.load(tmp_path / f"slice_rank{r}.npy")
        assert len(seen) == 1
        lo, hi, delivered = (int(v) for v in seen[0])
        slices.append((lo, hi))
        assert delivered == len(paths) * (hi - lo)
    assert slices[0][0] == 0 and slices[-1][1] == 4 ** 7 and all(a[1] == b[0] for a, b in zip(slices[:-1], slices[1:]))


def test_offline_tool(tmp_path, manifest):
    paths = _family(tmp_path, manifest, n=6)
    proj = str(tmp_path / "off")
    merger.merge(proj, paths, partial_fn=numpy_patterns_partial, windows=[(2, 255)], patterns=True)
    kmv = patterns.load(proj + ".002-255.kmv")
    names = patterns.table_names(kmv["meta"]["data"])
    assert len(set(names)) == 6
    for p in paths:                                                          # no .kin is needed from here on
        os.remove(p)
    env = dict(os.environ, PYTHONPATH=ROOT)
    p, cwd = kmv["patterns"], str(tmp_path)

    def tool(*argv, status=0):
        return run_py("-m", "pykmer_amd.patterns", "off.002-255.kmv", *argv, cwd=cwd, env=env, status=status)
    assert int(tool("--all-of", "0,1,2,3,4,5").stdout) == int(p[-1])
    assert int(tool("--all-of", "2", "--none-of", "0,1,3,4,5").stdout) == int(p[1 << 2])
    by_name = tool("--all-of", f"{names[0]},{names[3]}", "--none-of", names[5], "--any-of", f"1,{names[2]}")
    assert int(by_name.stdout) == patterns.count_where(p, 6, all_of=[0, 3], none_of=[5], any_of=[1, 2])
    assert int(tool("--any-of", "0,1,2,3,4,5").stdout) == 4 ** 7 - int(p[0])
    r = tool("--all-of", "0,nobody", status=1)
    assert r.stderr.startswith("error: ") and "nobody" in r.stderr and r.stdout == ""
    assert tool("--all-of", "6", status=1).stderr.startswith("error: ")
    tool("--kma", "again")
    with np.load(tmp_path / "again.002-255.kma") as a, np.load(proj + ".002-255.kma") as b:
        assert np.array_equal(a["matrix"], b["matrix"])
    assert json.load(open(tmp_path / "again.002-255.kma.json"))["data"] == kmv["meta"]["data"]
    assert tool("--kma", "again", status=1).stderr.startswith("error: ")     # not overwritten
    assert tool(status=2).stderr != ""                                       # nothing asked for


def test_refusals_leave_no_file(tmp_path, manifest, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    (tmp_path / "in").mkdir()
    paths = _family(tmp_path / "in", manifest, n=3)
    many = [str(tmp_path / "in" / f"x{i:02d}.kin") for i in range(17)]

    def outputs():
        return [f for f in os.listdir(tmp_path) if f != "in"]
    with pytest.raises(ValueError, match="1 to 16 tables, got 17"):
        merger.merge("p", many, partial_fn=numpy_patterns_partial, patterns=True)
    with pytest.raises(SystemExit) as e:
        merger.main(["p", *many, "--patterns"])
    out = capsys.readouterr().out
    assert e.value.code == 1 and "error: " in out and "16 tables" in out
    for extra in ("--kwip", "--spectrum"):
        with pytest.raises(SystemExit) as e:
            merger.main(["p", *paths, "--patterns", extra])
        assert e.value.code == 2 and "--patterns takes no" in capsys.readouterr().err
    with pytest.raises(AssertionError):
        merger.merge("p", paths, partial_fn=numpy_patterns_partial, patterns=True, kwip=True)
    with pytest.raises(AssertionError):
        merger.merge("p", paths, partial_fn=numpy_patterns_partial, patterns=True, spectrum=True)
    assert outputs() == []
    open("p.001-255.kmv", "wb").close()
    with pytest.raises(AssertionError, match="already exists"):
        merger.merge("p", paths, partial_fn=numpy_patterns_partial, patterns=True)
    assert outputs() == ["p.001-255.kmv"] and os.path.getsize("p.001-255.kmv") == 0
