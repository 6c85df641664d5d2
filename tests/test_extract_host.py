"""CPU: the extract path's argument checks, its growth / halving driver, its file writers and its two entry points.
No call here touches a GPU: staging and the device call are stood in for by numpy (extract_ref)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import extract_ref
from oracle import pyoracle
from host_support import stub_header
from pykmer_amd import _lib, extract

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ validate ----------------------
def test_validate_refuses_bad_arguments(tmp_path):
    a, b, c = stub_header(9, "a.kin"), stub_header(9, "b.kin"), stub_header(9, "c.kin")
    assert extract.validate([a, b], [c]) == (9, 2)
    assert extract.validate([a, b], [c], 2, 200, 1, 1) == (9, 1)
    with pytest.raises(ValueError, match="even.kin"):
        extract.validate([stub_header(8, "even.kin")], [])
    with pytest.raises(ValueError, match="d.kin.*differs"):
        extract.validate([a], [stub_header(11, "d.kin")])
    with pytest.raises(ValueError, match="at least one present"):
        extract.validate([], [a])
    many = [stub_header(9, f"t{i}.kin") for i in range(129)]
    assert extract.validate(many[:64], many[64:128]) == (9, 64)
    with pytest.raises(ValueError, match="at most 128"):
        extract.validate(many[:100], many[100:])
    for bad in (0, 3):
        with pytest.raises(ValueError, match="min_present"):
            extract.validate([a, b], [c], min_present=bad)
    with pytest.raises(ValueError, match="max_absent"):
        extract.validate([a, b], [c], max_absent=2)
    with pytest.raises(ValueError, match="max_absent"):
        extract.validate([a, b], [c], max_absent=-1)
    for mn, mx in ((0, 3), (1, 256), (5, 4)):
        with pytest.raises(ValueError, match="count window"):
            extract.validate([a], [], mn, mx)
    with pytest.raises(ValueError, match="named twice"):
        extract.validate([a, b], [stub_header(9, "a.kin")])
    with pytest.raises(ValueError, match="named twice"):
        extract.validate([a, stub_header(9, "./a.kin")], [])
    proj = str(tmp_path / "proj")
    assert extract.validate([a], [], project_name=proj) == (9, 1)
    for f in extract.kmx_paths(proj):
        f.write_bytes(b"")
        with pytest.raises(ValueError, match="already exists"):
            extract.validate([a], [], project_name=proj)
        with pytest.raises(ValueError, match="already exists"):
            extract.extract(proj, [tmp_path / "a.kin"])
        f.unlink()


# ------------------------------------------------------------------ growth and halving ------------
K = 7
PARAMS = dict(min_count=2, max_count=200, min_present=2, max_absent=1)


class _NumpyCall:
    """extract.DeviceCall's shape on host arrays: honours `cap` the way pk_extract_device does."""

    def __init__(self, n_present, text=False, params=None):
        self.P, self.text, self.log, self.params = n_present, text, [], params or PARAMS

    def __call__(self, ptrs, off, n, first_addr, cap):
        sl = [t[off:off + n] for t in ptrs]
        addr, counts = extract_ref.expected(sl[:self.P], sl[self.P:], self.params["min_count"], self.params["max_count"], self.params["min_present"],
                                            self.params["max_absent"], first_addr=first_addr)
        self.log.append((first_addr, n, cap, addr.size))
        if addr.size > cap:
            return addr.size, None
        return addr.size, (addr, counts, extract_ref.decode(addr, K) if self.text else None)


def _stage(piece):
    def stage(tables, lo, hi, device, threads, reserve, budget):
        for a in range(lo, hi, piece):
            b = min(hi, a + piece)
            yield [t.table[a:b] for t in tables], a, b
    return stage


@pytest.fixture(scope="module")
def small():
    dense = extract_ref.mixed_tables(4 ** K, 5, seed=7)
    tables = [stub_header(K, f"t{i}.kin", t) for i, t in enumerate(dense)]
    want = extract_ref.expected(dense[:3], dense[3:], PARAMS["min_count"], PARAMS["max_count"], PARAMS["min_present"], PARAMS["max_absent"])
    assert 2000 < want[0].size < 4 ** K // 2
    return tables, want


def _same(got, want):
    assert got["addr"].dtype == np.uint64 and got["counts"].dtype == np.uint8 and got["counts"].shape == (want[0].size, 3)
    assert np.array_equal(got["addr"], want[0]) and np.array_equal(got["counts"], want[1])
    assert (np.diff(got["addr"].astype(np.int64)) > 0).all() and got["n_selected"] == want[0].size


def test_capacity_grows_to_the_reported_count(small):
    tables, want = small
    call = _NumpyCall(3)
    got = extract.extract_kmers(tables[:3], tables[3:], **PARAMS, hbm_budget=1 << 30, initial_rows=5, stage=_stage(4 ** K), call=call)
    _same(got, want)
    assert call.log == [(0, 4 ** K, 5, want[0].size), (0, 4 ** K, want[0].size, want[0].size)] and got["n_calls"] == 2
    roomy = _NumpyCall(3)
    _same(extract.extract_kmers(tables[:3], tables[3:], **PARAMS, hbm_budget=1 << 30, stage=_stage(4 ** K), call=roomy), want)
    assert len(roomy.log) == 1


def test_pieces_halve_when_the_output_budget_is_small(small):
    tables, want = small
    dense = [t.table for t in tables]
    loose = dict(min_count=2, max_count=200, min_present=1, max_absent=2)
    for params, want in ((PARAMS, want), (loose, extract_ref.expected(dense[:3], dense[3:], 2, 200, 1, 2))):
        call = _NumpyCall(3, params=params)
        # a budget of 1 byte leaves the output its floor: exactly 2048 rows, fewer than either selection
        got = extract.extract_kmers(tables[:3], tables[3:], **params, hbm_budget=1, stage=_stage(10240), call=call)
        assert want[0].size > 2048
        _same(got, want)
        assert got["n_pieces"] == 2
        sizes = {n for _, n, _, _ in call.log}
        assert 10240 in sizes and min(sizes) >= 2048 and len(sizes) > 1        # some piece was halved
        assert all(first % 2048 == 0 and n % 2048 == 0 and cap <= 2048 for first, n, cap, _ in call.log)
        done = [(first, n) for first, n, cap, m in call.log if m <= cap]
        assert done == sorted(done) and sum(n for _, n in done) == 4 ** K      # the ranges that delivered tile the table, in order
        assert all(a + n == b for (a, n), (b, _) in zip(done, done[1:]))
    assert min(sizes) == 2048                                                # the loose selection goes down to the floor


def test_everything_selected_in_one_minimal_piece():
    """2048 addresses always fit: a piece of 2048 addresses that selects all of them is never halved."""
    t = stub_header(K, "full.kin", np.full(4 ** K, 9, dtype=np.uint8))
    params = dict(min_count=2, max_count=200, min_present=1, max_absent=0)
    call = _NumpyCall(1, params=params)
    got = extract.extract_kmers([t], [], **params, hbm_budget=1, initial_rows=1, stage=_stage(2048), call=call)
    assert np.array_equal(got["addr"], np.arange(4 ** K, dtype=np.uint64)) and (got["counts"] == 9).all()
    assert {n for _, n, _, _ in call.log} == {2048}


# ------------------------------------------------------------------ files -------------------------
def test_file_round_trip(small, tmp_path):
    tables, want = small
    got = extract.extract_kmers(tables[:3], tables[3:], **PARAMS, hbm_budget=1 << 30, text=True, stage=_stage(5000), call=_NumpyCall(3, text=True))
    _same(got, want)
    proj = str(tmp_path / "proj")
    data = [{"pos": i, "role": "present" if i < 3 else "absent", "index_file": tmp_path / f"t{i}.kin", "description_file": tmp_path / f"t{i}.kin.json",
             "header": {"kmer_len": K}} for i in range(5)]
    extract.write_kmx(proj, got, data)
    assert not list(tmp_path.glob("*.tmp"))
    z = np.load(proj + ".kmx")
    scalars = {"kmer_len": K, "min_count": 2, "max_count": 200, "min_present": 2, "max_absent": 1, "n_present": 3, "n_absent": 2}
    assert sorted(z.files) == sorted(["addr", "counts"] + list(scalars))
    assert z["addr"].dtype == np.uint64 and z["addr"].shape == (want[0].size,) and np.array_equal(z["addr"], want[0])
    assert z["counts"].dtype == np.uint8 and z["counts"].shape == (want[0].size, 3) and np.array_equal(z["counts"], want[1])
    for key, v in scalars.items():
        assert z[key].shape == () and int(z[key]) == v, key
    with open(proj + ".kmx.json") as fh:
        meta = json.load(fh)
    assert sorted(meta) == sorted(["data", "n_selected", "project_name"] + list(scalars))
    assert meta["n_selected"] == want[0].size and all(meta[key] == v for key, v in scalars.items())
    assert [d["role"] for d in meta["data"]] == ["present"] * 3 + ["absent"] * 2 and [d["pos"] for d in meta["data"]] == list(range(5))
    assert [d["index_file"] for d in meta["data"]] == [str(tmp_path / f"t{i}.kin") for i in range(5)]
    text = open(proj + ".kmx.txt", "rb").read()
    assert text == extract_ref.decode(want[0], K).tobytes()
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines) == want[0].size + 1 and all(len(ln) == K for ln in lines[:-1])
    # without the text no .kmx.txt is written
    other = str(tmp_path / "plain")
    extract.write_kmx(other, {key: v for key, v in got.items() if key != "text"}, data)
    assert os.path.exists(other + ".kmx") and not os.path.exists(other + ".kmx.txt")


def test_letters_invert_the_indexers_encoding():
    """Codes 0,1,2,3 = A,C,G,T, first base in the highest bits -- the rule the reference's README states and its indexer
    applies (indexer.py:131: weight 4^(k-p-1) for base p), so AAACC = 0*256 + 0*64 + 0*16 + 1*4 + 1 = 5.  The README's worked
    example `AACC = 40` does not follow that rule (it codes C as 2 and weighs the last base by 4); the same arithmetic on
    AAACC would give 40, which by the rule that addresses a .kin is AAGGA.  Both are pinned here."""
    assert extract_ref.decode([5], 5).tobytes() == b"AAACC\n"
    assert extract_ref.decode([40], 5).tobytes() == b"AAGGA\n"
    for word in ("AAACC", "AAGGA", "TTTTT", "ACGTA"):
        seq = tuple("ACGT".index(ch) for ch in word)
        (_, fwd, _), = pyoracle.windows(seq, 5)
        assert extract_ref.decode([fwd], 5).tobytes() == word.encode() + b"\n"
    assert extract_ref.decode([0, 4 ** 17 - 1], 17).tobytes() == b"A" * 17 + b"\n" + b"T" * 17 + b"\n"


# ------------------------------------------------------------------ entry points ------------------
def test_header_declares_and_library_exports_the_entry_points():
    names = ("pk_extract_device", "pk_extract_text")
    text = open(os.path.join(ROOT, "include", "pykmer_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()[-2] in "TW"}
    lib = _lib.load()
    for name in names:
        assert name in declared and name in exported and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.pk_version() == 3
