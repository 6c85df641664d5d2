"""CPU: the table output of the extract path (combine_tables, extract.py --table): how the pieces are assembled, what is
refused, the `.kin.json` of a derived table and the entry point behind it.  No call here touches a GPU: staging and the
device call are stood in for by numpy (combine_ref)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import combine_ref
import extract_ref
import oracle
from host_support import stub_header, write_kin
from pykmer_amd import _lib, extract
from pykmer_amd.header import Header, HeaderVars, gen_checksum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 7
PARAMS = dict(min_count=2, max_count=200, min_present=1, max_absent=0)


class _NumpyCall:
    """extract.TableCall's shape on host arrays."""

    def __init__(self, n_present, op, params=PARAMS, fail_at=None):
        self.P, self.op, self.params, self.fail_at = n_present, op, params, fail_at
        self.hist, self.log = np.zeros(256, dtype=np.uint64), []

    def __call__(self, ptrs, a, b, out):
        if self.fail_at is not None and len(self.log) == self.fail_at:
            raise RuntimeError("the device call failed")
        self.log.append((a, b))
        assert all(t.size == b - a for t in ptrs)
        piece = combine_ref.expected(ptrs[:self.P], ptrs[self.P:], self.op, **self.params)
        out[a:b] = piece
        self.hist += combine_ref.hist256(piece)

    def hist256(self):
        return self.hist


class _Stage:
    """Pieces of `piece` addresses as slices of the host tables; records what it was asked for and that it was closed."""

    def __init__(self, piece):
        self.piece, self.asked, self.open, self.closed = piece, None, 0, 0

    def __call__(self, tables, lo, hi, device, threads, reserve, budget):
        self.asked = (len(tables), lo, hi, reserve, budget)
        self.open += 1
        try:
            for a in range(lo, hi, self.piece):
                b = min(hi, a + self.piece)
                yield [t.table[a:b] for t in tables], a, b
        finally:
            self.closed += 1


@pytest.fixture(scope="module")
def small():
    """Three present tables and an absent one at k = 7, and what they exercise."""
    dense = extract_ref.mixed_tables(4 ** K, 4, seed=7, zero=0.3)
    prof = combine_ref.profile(dense[:3], dense[3:], **PARAMS)
    assert prof["saturated"] > 100 and prof["unsaturated"] > 1000 and prof["mixed"] > 500 and prof["occupancies"] == {1, 2, 3}
    return [stub_header(K, f"t{i}.kin", t) for i, t in enumerate(dense)], dense


# ------------------------------------------------------------------ the reference itself ----------
def test_reference_agrees_with_the_list_reference():
    assert combine_ref.OPS == extract.OPS                     # the ops of the tool are the ops of the definition
    tables = extract_ref.mixed_tables(4 ** 7 + 17, 4, seed=7, zero=0.3)
    prof = combine_ref.profile(tables[:3], tables[3:], 2, 200, 1, 0)
    assert 3000 < prof["selected"] < 4000 and prof["saturated"] > 100 and prof["unsaturated"] > 1000 and prof["mixed"] > 500
    assert prof["occupancies"] == {1, 2, 3}
    addr, counts = extract_ref.expected(tables[:3], tables[3:], 2, 200, 1, 0)
    for op in combine_ref.OPS:
        got = combine_ref.expected(tables[:3], tables[3:], op, 2, 200, 1, 0)
        assert got.dtype == np.uint8 and np.array_equal(np.flatnonzero(got).astype(np.uint64), addr), op
    one = combine_ref.expected(tables[:1], tables[3:], "max", 2, 200)
    addr, counts = extract_ref.expected(tables[:1], tables[3:], 2, 200)
    assert np.array_equal(one[addr.astype(np.int64)], counts[:, 0])            # P = 1: the rows are inside the window
    # the identity of min: a zero, a byte below the window and one inside it
    tri = [np.array([0], np.uint8), np.array([1], np.uint8), np.array([9], np.uint8)]
    assert [int(combine_ref.expected(tri, [], op, 2, 200, 1)[0]) for op in combine_ref.OPS] == [9, 9, 9, 1]


# ------------------------------------------------------------------ combine_tables ----------------
@pytest.mark.parametrize("op", combine_ref.OPS)
def test_pieces_are_assembled_at_their_offsets(small, op):
    tables, dense = small
    want = combine_ref.expected(dense[:3], dense[3:], op, **PARAMS)
    stage, call = _Stage(5000), _NumpyCall(3, op)
    got = extract.combine_tables(tables[:3], tables[3:], op=op, **PARAMS, hbm_budget=1 << 20, stage=stage, call=call)
    assert got["table"].dtype == np.uint8 and np.array_equal(got["table"], want)
    assert got["n_pieces"] == 4 and call.log == [(0, 5000), (5000, 10000), (10000, 15000), (15000, 4 ** K)]
    assert stage.asked == (4, 0, 4 ** K, extract.HIST_BYTES, 1 << 20) and (stage.open, stage.closed) == (1, 1)
    assert np.array_equal(got["hist256"], combine_ref.hist256(want)) and got["hist256"].dtype == np.uint64
    assert got["n_selected"] == np.count_nonzero(want) == extract_ref.select_mask(dense[:3], dense[3:], **PARAMS).sum()
    assert (got["op"], got["kmer_len"], got["n_present"], got["n_absent"]) == (op, K, 3, 1)
    assert (got["min_count"], got["max_count"], got["min_present"], got["max_absent"]) == (2, 200, 1, 0)
    out = np.full(4 ** K, 0xA5, dtype=np.uint8)                                  # the caller's array is the one filled
    again = extract.combine_tables(tables[:3], tables[3:], op=op, **PARAMS, out=out, stage=_Stage(4 ** K), call=_NumpyCall(3, op))
    assert again["table"] is out and np.array_equal(out, want) and again["n_pieces"] == 1


def test_staging_is_released_when_the_call_raises(small):
    tables, dense = small
    stage = _Stage(5000)
    with pytest.raises(RuntimeError, match="device call failed"):
        extract.combine_tables(tables[:3], tables[3:], op="sum", **PARAMS, stage=stage, call=_NumpyCall(3, "sum", fail_at=2))
    assert (stage.open, stage.closed) == (1, 1)


def test_own_buffers_are_freed_on_every_exit_path(small, monkeypatch):
    """Without `call=` combine_tables makes a TableCall of its own and frees its device buffers, also when the pass fails."""
    tables, dense = small
    made = []

    class Buf:
        def __init__(self, n, device=0):
            self.n, self.ptr, self.freed = n, 4096, False
            made.append(self)

        def zero(self):
            pass

        def free(self):
            self.freed = True

    def device_call(*a, **kw):
        raise RuntimeError("no device here")
    monkeypatch.setattr(extract._lib, "DeviceBuffer", Buf)
    monkeypatch.setattr(extract._lib, "extract_table_device", device_call)
    stage = _Stage(5000)
    with pytest.raises(RuntimeError, match="no device here"):
        extract.combine_tables(tables[:3], tables[3:], op="max", **PARAMS, stage=stage)
    assert sorted(b.n for b in made) == [extract.HIST_BYTES, 5008] and all(b.freed for b in made) and stage.closed == 1


def test_combine_refuses_bad_arguments(small):
    tables, dense = small
    for op in ("avg", "SUM", "", None, 0):
        with pytest.raises(ValueError, match="unknown table operation"):
            extract.combine_tables(tables[:3], tables[3:], op=op, stage=_Stage(5000), call=_NumpyCall(3, "sum"))
    with pytest.raises(ValueError, match="min_present"):
        extract.combine_tables(tables[:3], tables[3:], op="sum", min_present=4, stage=_Stage(5000), call=_NumpyCall(3, "sum"))
    with pytest.raises(ValueError, match="count window"):
        extract.combine_tables(tables[:3], [], op="sum", min_count=0, stage=_Stage(5000), call=_NumpyCall(3, "sum"))
    for bad in (np.zeros(4 ** K - 1, np.uint8), np.zeros(4 ** K, np.int8), np.zeros(2 * 4 ** K, np.uint8)[::2]):
        with pytest.raises(ValueError, match="out must be"):
            extract.combine_tables(tables[:3], tables[3:], op="sum", out=bad, stage=_Stage(5000), call=_NumpyCall(3, "sum"))
    assert extract.OPS == ("sum", "min", "max", "count") == combine_ref.OPS
    assert extract.build_parser().parse_args(["p", "--present", "a.kin", "--table", "min"]).table == "min"
    assert extract.build_parser().parse_args(["p", "--present", "a.kin"]).table is None
    with pytest.raises(SystemExit):
        extract.build_parser().parse_args(["p", "--present", "a.kin", "--table", "avg"])


# ------------------------------------------------------------------ files -------------------------
def _fasta(seed, n=3000):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    seq = bytes(letters[rng.integers(0, 4, n)])
    unit = bytes(letters[np.random.default_rng(100).integers(0, 4, 40)]) if seed < 2 else seq[:40]   # samples 0 and 1 share a repeat: 150 + 150 > 255
    return b">s%d\n" % seed + seq + b"\n>rep\n" + unit * 150 + b"\n"


@pytest.fixture()
def project(tmp_path):
    written = [write_kin(tmp_path, f"s{i}.fa", _fasta(i), K, project=f"s{i}.fa") for i in range(3)]
    kins, tables = [w.path for w in written], [w.table for w in written]
    data = []
    for i, kin in enumerate(kins):
        data.append({"pos": i, "role": "present" if i < 2 else "absent", "index_file": kin, "description_file": kin + ".json",
                     "header": Header(kin, index_file=kin)})
    return tmp_path, list(kins), list(tables), data


def _host_tables(data):
    """The stage of a run on files without a device: every Header's table read whole."""
    def stage(tables, lo, hi, device, threads, reserve, budget):
        yield [t.read_table_slice(lo, hi) for t in tables], lo, hi
    return stage


def test_table_files_and_their_json(project):
    tmp_path, kins, tables, data = project
    proj = str(tmp_path / "pooled")
    params = dict(min_count=1, max_count=255, min_present=1, max_absent=0)
    want = combine_ref.expected(tables[:2], tables[2:], "sum", **params)
    assert (want == 255).any() and 0 < np.count_nonzero(want) < want.size
    result = extract.write_table(proj, "sum", data, 0, **params, stage=_host_tables(data), call=_NumpyCall(2, "sum", params))
    kin, meta_file, kmx_json = (str(p) for p in extract.table_paths(proj, K))
    assert (kin, meta_file, kmx_json) == (proj + ".07.kin", proj + ".07.kin.json", proj + ".kmx.json") and result["table_file"] == kin
    assert sorted(p.name for p in tmp_path.glob("pooled*")) == ["pooled.07.kin", "pooled.07.kin.json", "pooled.kmx.json"]
    assert not list(tmp_path.glob("*.tmp"))
    assert np.array_equal(np.fromfile(kin, dtype=np.uint8), want) and result["n_selected"] == np.count_nonzero(want)
    with open(meta_file) as fh:
        text = fh.read()
    meta = json.loads(text)
    assert sorted(meta) == sorted(HeaderVars.HEADER_FIXED + HeaderVars.HEADER_DATA) and len(meta) == 33
    assert text == json.dumps(meta, indent=1, sort_keys=True)
    assert meta["input_file_size"] is None and meta["input_file_ctime"] is None and meta["input_file_cheksum"] is None
    assert (meta["project_name"], meta["input_file_name"], meta["input_file_path"]) == ("pooled", "pooled", proj)
    fresh = Header("pooled", input_file=proj, kmer_len=K)
    assert (meta["kmer_len"], meta["flush_every"], meta["frag_size"]) == (K, fresh.flush_every, fresh.frag_size)
    assert (meta["file_ver"], meta["kmer_size"], meta["data_size"], meta["max_size"]) == ("KMER001", 4 ** K, 4 ** K, 4 ** K)
    assert meta["output_file_size"] == 4 ** K == os.path.getsize(kin) and meta["output_file_cheksum"] == gen_checksum(kin)
    assert isinstance(meta["output_file_ctime"], float) and isinstance(meta["hostname"], str) and isinstance(meta["creation_speed"], int)
    assert meta["checksum_script"] == gen_checksum(os.path.join(ROOT, "pykmer_amd", "header.py"))
    assert all(isinstance(meta[f], str) for f in ("creation_time_start", "creation_time_end", "creation_duration"))
    assert meta["num_kmers"] == meta["vals_sum"] == int(want.sum(dtype=np.uint64)) > 0
    ref_hist, _ = np.histogram(want, bins=255, range=(1, 255))
    assert meta["hist"] == ref_hist.tolist() and meta["vals_count"] == np.count_nonzero(want) and meta["vals_max"] == 255
    heads = [v["header"] for v in data]                       # lean dicts by now
    assert meta["chromosomes"] == [["present:s0.fa", heads[0]["num_kmers"]], ["present:s1.fa", heads[1]["num_kmers"]],
                                   ["absent:s2.fa", heads[2]["num_kmers"]]]
    loaded = Header(kin, index_file=kin)                      # the consumer contract of every tool
    assert loaded.kmer_len == K and loaded.num_kmers == meta["num_kmers"] and loaded.input_file_name == "pooled"
    assert loaded.index_file == kin and np.array_equal(loaded.read_table(), want)
    lean = loaded.to_dict(lean=True)
    assert "chromosomes" not in lean and len(lean) == 32
    with open(kmx_json) as fh:
        kmx = json.load(fh)
    scalars = {"kmer_len": K, "min_count": 1, "max_count": 255, "min_present": 1, "max_absent": 0, "n_present": 2, "n_absent": 1}
    assert sorted(kmx) == sorted(["data", "n_selected", "project_name", "table", "table_file"] + list(scalars))
    assert kmx["table"] == "sum" and kmx["table_file"] == kin and kmx["n_selected"] == np.count_nonzero(want)
    assert all(kmx[key] == v for key, v in scalars.items()) and [d["role"] for d in kmx["data"]] == ["present", "present", "absent"]
    assert [d["index_file"] for d in kmx["data"]] == kins
    # the derived table is a table like any other: it goes back in
    again = extract.combine_tables([loaded], [Header(kins[2], index_file=kins[2])], op="max", stage=_host_tables(None), call=_NumpyCall(1, "max", params))
    assert np.array_equal(again["table"], combine_ref.expected([want], tables[2:], "max"))


def test_empty_selection_leaves_no_file(project):
    tmp_path, kins, tables, data = project
    assert not (tables[0] == 254).any()
    before = sorted(p.name for p in tmp_path.iterdir())
    params = dict(min_count=254, max_count=254, min_present=None, max_absent=0)
    with pytest.raises(ValueError, match=r"no k-mer is selected \(count window 254-254, min_present 1 of 1, max_absent 0 of 0\)"):
        extract.write_table(str(tmp_path / "none"), "max", data[:1], 0, **params, stage=_host_tables(data),
                            call=_NumpyCall(1, "max", dict(params, min_present=1)))
    assert sorted(p.name for p in tmp_path.iterdir()) == before


def test_failed_pass_leaves_no_file(project):
    tmp_path, kins, tables, data = project
    before = sorted(p.name for p in tmp_path.iterdir())
    with pytest.raises(RuntimeError, match="device call failed"):
        extract.write_table(str(tmp_path / "broken"), "sum", data, 0, stage=_host_tables(data), call=_NumpyCall(2, "sum", fail_at=0))
    assert sorted(p.name for p in tmp_path.iterdir()) == before


def test_table_run_refuses_to_overwrite_and_to_list_kmers(project, capsys):
    tmp_path, kins, tables, data = project
    proj = str(tmp_path / "proj")
    for f in extract.table_paths(proj, K) + (tmp_path / "proj.07.kin.bgz",):
        f.write_bytes(b"x")
        before = sorted(p.name for p in tmp_path.iterdir())
        with pytest.raises(ValueError, match="already exists"):
            extract.extract(proj, kins[:2], kins[2:], table="sum")
        with pytest.raises(SystemExit) as exit_:
            extract.main([proj, "--present", kins[0], kins[1], "--absent", kins[2], "--table", "sum"])
        assert exit_.value.code == 1 and "error:" in capsys.readouterr().err
        assert sorted(p.name for p in tmp_path.iterdir()) == before and f.read_bytes() == b"x"
        f.unlink()
    (tmp_path / "proj.kmx").write_bytes(b"x")                 # a list of the same project is not in a table's way ...
    with pytest.raises(ValueError, match="cannot be combined with --kmers"):
        extract.extract(proj, kins[:2], kins[2:], kmers=True, table="sum")
    with pytest.raises(SystemExit) as exit_:
        extract.main([proj, "--present", kins[0], "--table", "sum", "--kmers"])
    assert exit_.value.code == 1 and "--kmers" in capsys.readouterr().err
    with pytest.raises(ValueError, match="unknown table operation"):
        extract.extract(proj, kins[:2], table="mean")
    with pytest.raises(ValueError, match="named twice"):
        extract.extract(proj, kins[:1], kins[:1], table="max")
    with pytest.raises(ValueError, match="already exists"):    # ... and without --table everything is as it was
        extract.extract(proj, kins[:2])


# ------------------------------------------------------------------ the pooling identity ----------
def test_saturating_sum_is_the_table_of_the_pooled_files():
    """min(255, sum of min(255, c_i)) = min(255, sum of c_i): the sum of the per-file tables is the table of the files
    counted as one.  The records of x and y do not join: x ends in a newline and y begins with a header."""
    k = 7
    rng = np.random.default_rng(11)
    letters = np.frombuffer(b"ACGT", np.uint8)
    unit, unit2 = bytes(letters[rng.integers(0, 4, 40)]), bytes(letters[rng.integers(0, 4, 40)])
    body = bytes(letters[rng.integers(0, 4, 5000)])
    x = b">x1\n" + body + b"\n>x2\n" + unit * 200 + b"\n>x3\n" + unit2 * 300 + b"\n"
    y = b">y1\n" + body[1000:3000] + b"\n>y2\n" + unit * 100 + b"\nACGT\n"
    tx, ty = oracle.count_fasta(x, k)["table"], oracle.count_fasta(y, k)["table"]
    raw = tx.astype(np.int64) + ty
    assert ((raw > 255) & (tx < 255) & (ty < 255)).any() and (tx == 255).any() and ((raw > 1) & (raw < 255)).any()
    pooled = combine_ref.expected([tx, ty], [], "sum", 1, 255, 1, 0)
    assert np.array_equal(pooled, oracle.count_fasta(x + y, k)["table"])
    assert np.array_equal(pooled, np.minimum(255, raw).astype(np.uint8))
    tabs = [stub_header(k, "x.kin", tx), stub_header(k, "y.kin", ty)]      # the pooling recipe: --present x y --min-present 1 --table sum
    got = extract.combine_tables(tabs, op="sum", min_present=1, stage=_Stage(4 ** k), call=_NumpyCall(2, "sum", dict(min_present=1)))
    assert np.array_equal(got["table"], pooled) and got["n_selected"] == np.count_nonzero(raw)


# ------------------------------------------------------------------ the entry point ---------------
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "pykmer_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", code))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()[-2] in "TW"}
    lib = _lib.load()
    name = "pk_extract_table_device"
    assert name in declared and name in exported and name in _lib.EXPORTS and hasattr(lib, name)
    assert re.search(r"PK_TABLE_SUM = 0, PK_TABLE_MIN = 1, PK_TABLE_MAX = 2, PK_TABLE_COUNT = 3", code)
    assert _lib.TABLE_OPS == ("sum", "min", "max", "count")
    assert lib.pk_version() == 3
