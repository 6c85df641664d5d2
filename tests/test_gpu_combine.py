"""GPU: the table kernel (kmer_extract.hip k_extract_table, pk_extract_table_device) and the host path above it
(combine_tables, extract.py --table) against the numpy restatement (combine_ref); exact equality everywhere."""
import ctypes
import json
import os

import numpy as np
import pytest

import gpu_support as gs
import combine_ref
import extract_ref
import inputs
import oracle
import query_ref
import synth
from gpu_support import ROOT, SENTINEL, Device, HostTable, SentinelOut, lib, run_py

pytestmark = pytest.mark.gpu
OPS = combine_ref.OPS


class _Out(SentinelOut):
    """A sentinel-filled output table of `size` bytes and a zeroed histogram accumulator in HBM."""

    def __init__(self, size):
        super().__init__(table=(max(16, size) + 15) & ~15)
        self.hist = lib().DeviceBuffer(256 * 8, 0)
        self.hist.zero()

    def untouched(self):
        return super().untouched() and not self.hist.download().any()

    def hist256(self, addresses):
        """The accumulator with the zeros filled in: the device tallies the values 1 .. 255."""
        h = self.hist.download().view(np.uint64).copy()
        assert h[0] == 0
        h[0] = addresses - int(h[1:].sum())
        return h

    def free(self):
        super().free()
        self.hist.free()


def _check(present, absent, op, mn=1, mx=255, min_present=None, max_absent=0, n=None, ptrs=None):
    """One pk_extract_table_device call on the first n addresses into a sentinel-filled table longer than n: bytes [0, n)
    equal the reference, every byte behind them is untouched, the histogram is the bincount of the result."""
    P = len(present)
    n = present[0].size if n is None else n
    min_present = P if min_present is None else min_present
    want = combine_ref.expected([t[:n] for t in present], [t[:n] for t in absent], op, mn, mx, min_present, max_absent)
    out = _Out(n + 64)
    try:
        if ptrs is None:
            with Device(list(present) + list(absent), min_bytes=16) as dev:
                secs = lib().extract_table_device(dev.ptrs, P, n, mn, mx, min_present, max_absent, op, out.table.ptr, out.hist.ptr)
        else:
            secs = lib().extract_table_device(ptrs, P, n, mn, mx, min_present, max_absent, op, out.table.ptr, out.hist.ptr)
        got = out.table.download()
        assert secs > 0
        assert np.array_equal(got[:n], want), (op, np.flatnonzero(got[:n] != want)[:5], got[:n][got[:n] != want][:5], want[got[:n] != want][:5])
        assert (got[n:] == SENTINEL).all(), op
        assert np.array_equal(out.hist256(n), combine_ref.hist256(want)), op
    finally:
        out.free()
    return want


# ------------------------------------------------------------------ 1. slice sizes x op ------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 1023, 1024, 2049, 4 ** 7, 4 ** 7 + 17])
def test_slice_sizes(gpu, n):
    """The tables are longer than the slice and hold selectable bytes behind it: nothing at or beyond n_slice is read as
    data or written.  4^7 + 17 addresses are two workgroups, the second one 17 addresses long."""
    tables = extract_ref.mixed_tables(n + 64, 4, seed=n, zero=0.3)
    for t in tables[:3]:
        t[n:] = 100
    tables[3][n:] = 0
    if n >= 4 ** 7:
        prof = combine_ref.profile([t[:n] for t in tables[:3]], [t[:n] for t in tables[3:]], 2, 200, 1, 0)
        assert prof["saturated"] > 100 and prof["unsaturated"] > 1000 and prof["mixed"] > 500 and prof["occupancies"] == {1, 2, 3}, prof
    with Device(tables, min_bytes=16) as dev:
        for op in OPS:
            want = _check(tables[:3], tables[3:], op, 2, 200, 1, 0, n=n, ptrs=dev.ptrs)
            assert n < 64 or 0 < np.count_nonzero(want) < n


# ------------------------------------------------------------------ 2. window edges ----------------
@pytest.mark.parametrize("mn,mx", [(2, 200), (1, 255), (128, 129), (127, 127), (255, 255), (2, 254)])
def test_window_edges(gpu, mn, mx):
    edge = np.array(sorted({max(mn - 1, 0), mn, mx, min(mx + 1, 255), 0, 255, 1, 127, 128}), dtype=np.uint8)
    m = edge.size
    a, b, c = np.repeat(edge, m * m), np.tile(np.repeat(edge, m), m), np.tile(edge, m * m)     # every triple of edge values
    absent = np.zeros(a.size, dtype=np.uint8)
    absent[2::5] = 1                                         # count 1 is held, whatever the window
    absent[1::7] = 255
    with Device([a, b, c, absent], min_bytes=16) as dev:
        for op in OPS:
            for min_present in (1, 3):
                want = _check([a, b, c], [absent], op, mn, mx, min_present, 0, ptrs=dev.ptrs)
                assert 0 < np.count_nonzero(want) < a.size


# ------------------------------------------------------------------ 3. 128 tables ------------------
def test_counters_and_sums_at_128_tables(gpu):
    n = 4100
    for value, want_sum in ((1, 128), (2, 255), (255, 255)):  # 128, 256 clamped, 32 640 clamped: a wrap in 8 or 15 bits shows
        full = [np.full(n, value, dtype=np.uint8)] * 128
        with Device(full[:1], min_bytes=16) as dev:                        # the same slice 128 times: the kernel reads 128 pointers
            ptrs = dev.ptrs * 128
            assert (_check(full, [], "sum", ptrs=ptrs) == want_sum).all()
            assert (_check(full, [], "count", ptrs=ptrs) == 128).all()
            assert (_check(full, [], "min", ptrs=ptrs) == value).all() and (_check(full, [], "max", ptrs=ptrs) == value).all()
    tables = extract_ref.mixed_tables(n, 128, seed=3, zero=0.5)
    with Device(tables, min_bytes=16) as dev:
        for op in OPS:
            want = _check(tables[:127], tables[127:], op, 2, 200, 40, 0, ptrs=dev.ptrs)
            assert 0 < np.count_nonzero(want) < n
        count = _check(tables, [], "count", 1, 255, 1, 0, ptrs=dev.ptrs)
        assert count.max() > 64 and (_check(tables, [], "sum", 1, 255, 1, 0, ptrs=dev.ptrs) == 255).any()


# ------------------------------------------------------------------ 4. the identity of min ---------
def test_bytes_outside_the_window_take_no_part(gpu):
    """An address where one present byte is 0, one lies below the window and one inside it, in every order of the three
    tables and at every position of a thread's 16 bytes; and the same with a byte above the window."""
    n = 96
    for outside in (1, 201):
        for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
            trio = [np.zeros(n, np.uint8), np.full(n, outside, np.uint8), (np.arange(n) % 150 + 2).astype(np.uint8)]
            present = [trio[i] for i in order]
            inside = trio[2]
            assert (_check(present, [], "min", 2, 200, 1) == inside).all() and (_check(present, [], "max", 2, 200, 1) == inside).all()
            assert (_check(present, [], "sum", 2, 200, 1) == inside).all() and (_check(present, [], "count", 2, 200, 1) == 1).all()


# ------------------------------------------------------------------ 5. the histogram accumulates ---
def test_histogram_accumulates_over_the_slices_of_a_table(gpu):
    n, cut = 3 * 2048 + 17, 2 * 2048
    tables = extract_ref.mixed_tables(n, 3, seed=5, zero=0.3)
    want = combine_ref.expected(tables[:2], tables[2:], "sum", 2, 200, 1, 0)
    out = _Out(n)
    with Device(tables, min_bytes=16) as dev:
        lib = gs.lib()
        lib.extract_table_device(dev.ptrs, 2, cut, 2, 200, 1, 0, "sum", out.table.ptr, out.hist.ptr)
        first = out.hist256(cut)
        assert np.array_equal(first, combine_ref.hist256(want[:cut]))
        lib.extract_table_device([p + cut for p in dev.ptrs], 2, n - cut, 2, 200, 1, 0, "sum", out.table.ptr + cut, out.hist.ptr)
    assert np.array_equal(out.table.download(n), want)
    assert np.array_equal(out.hist256(n), combine_ref.hist256(want)) and (out.hist256(n)[1:] >= first[1:]).all()
    out.free()


# ------------------------------------------------------------------ 6. agreement with the list -----
@pytest.mark.parametrize("params", [(2, 200, 2, 1), (1, 255, 1, 0)])
def test_nonzero_addresses_are_the_extracted_list(gpu, params):
    from pykmer_amd import extract, merger
    k = 7
    tables = extract_ref.mixed_tables(4 ** k, 4, seed=6, zero=0.3)
    mn, mx, min_present, max_absent = params
    with Device(tables, min_bytes=16) as dev:
        resident = [merger.ResidentTable(p, 4 ** k, 4 ** k) for p in dev.ptrs]
        listed = extract.extract_kmers(resident[:2], resident[2:], mn, mx, min_present, max_absent)
        assert 100 < listed["n_selected"] < 4 ** k
        for op in OPS:
            got = extract.combine_tables(resident[:2], resident[2:], op, mn, mx, min_present, max_absent)
            assert np.array_equal(np.flatnonzero(got["table"]).astype(np.uint64), listed["addr"]) and got["n_selected"] == listed["n_selected"]
            assert np.array_equal(got["table"], combine_ref.expected(tables[:2], tables[2:], op, mn, mx, min_present, max_absent))
        one = extract.extract_kmers(resident[:1], resident[2:], mn, mx, 1, max_absent)
        got = extract.combine_tables(resident[:1], resident[2:], "max", mn, mx, 1, max_absent)
        assert np.array_equal(got["table"][one["addr"].astype(np.int64)], one["counts"][:, 0]) and got["n_selected"] == one["n_selected"]


# ------------------------------------------------------------------ 7. one larger slice ------------
def test_thousands_of_workgroups(gpu):
    """4^13 + 17 addresses: 4097 workgroups, the last one 17 addresses long."""
    n = 4 ** 13 + 17
    tables = extract_ref.mixed_tables(n, 3, seed=13, zero=0.3)
    want = _check(tables[:2], tables[2:], "sum", 2, 200, 1, 0)
    assert want[-17:].any() and (want == 255).any() and n // 8 < np.count_nonzero(want) < n // 4    # 0.58 of the addresses valid, 0.3 of those not absent


# ------------------------------------------------------------------ 8. arguments -------------------
def test_bad_arguments_are_refused(gpu):
    lib = gs.lib()
    n = 4096
    t = np.full(n, 3, dtype=np.uint8)
    with Device([t], min_bytes=16) as dev:
        p = dev.ptrs[0]
        out = _Out(n)

        def rc(tabs, P, A, mn=1, mx=255, minp=1, maxa=0, op=0, table=out.table.ptr, hist=out.hist.ptr, n_slice=n):
            ptrs = (ctypes.c_void_p * max(1, len(tabs)))(*tabs) if tabs is not None else None
            return lib.load().pk_extract_table_device(ptrs, P, A, n_slice, mn, mx, minp, maxa, op, ctypes.c_void_p(table) if table else None,
                                                      ctypes.c_void_p(hist) if hist else None, 0, None)
        for op in (-1, 4, 255):
            assert rc([p], 1, 0, op=op) == lib.PK_ERR_ARG
        assert rc([p], 1, 0, table=None) == lib.PK_ERR_ARG and rc([p], 1, 0, hist=None) == lib.PK_ERR_ARG
        assert rc([p], 1, 0, table=out.table.ptr + 1) == lib.PK_ERR_ARG and rc([p], 1, 0, table=out.table.ptr + 8) == lib.PK_ERR_ARG
        assert rc([p], 1, 0, hist=out.hist.ptr + 4) == lib.PK_ERR_ARG
        assert rc([p], 1, 0, table=p) == lib.PK_ERR_ARG and rc([p], 1, 0, table=p + n - 16) == lib.PK_ERR_ARG   # the output overlaps an input
        assert rc([p] * 129, 129, 0, minp=129) == lib.PK_ERR_ARG
        assert rc([p] * 129, 100, 29, minp=100) == lib.PK_ERR_ARG
        assert rc([p], 0, 1) == lib.PK_ERR_ARG
        assert rc([p], 1, -1) == lib.PK_ERR_ARG
        for mn, mx in ((0, 3), (1, 256), (5, 4)):
            assert rc([p], 1, 0, mn=mn, mx=mx) == lib.PK_ERR_ARG
        assert rc([p, p], 2, 0, minp=0) == lib.PK_ERR_ARG and rc([p, p], 2, 0, minp=3) == lib.PK_ERR_ARG
        assert rc([p, p], 1, 1, maxa=2) == lib.PK_ERR_ARG and rc([p, p], 1, 1, maxa=-1) == lib.PK_ERR_ARG
        assert rc([p, None], 1, 1) == lib.PK_ERR_ARG and rc(None, 1, 0) == lib.PK_ERR_ARG
        assert rc([p + 1], 1, 0) == lib.PK_ERR_ARG            # 16-byte alignment
        assert rc([p], 1, 0, n_slice=(1 << 40) + 1) == lib.PK_ERR_ARG
        assert out.untouched()
        with pytest.raises(ValueError, match="op must be"):
            lib.extract_table_device([p], 1, n, 1, 255, 1, 0, 7, out.table.ptr, out.hist.ptr)
        assert rc([p], 1, 0, n_slice=0) == lib.PK_OK and out.untouched()          # an empty slice: nothing is touched
        assert rc([p], 1, 0) == lib.PK_OK                                           # and a good call still works
        assert (out.table.download(n) == 3).all() and out.hist256(n)[3] == n
        out.free()


# ------------------------------------------------------------------ 9. the whole path, small -------
def test_whole_path_under_a_small_budget(gpu, monkeypatch):
    from pykmer_amd import extract
    k = 9
    x, y = inputs.record_dense_fasta(27 + 61 * 1000, 9, seed=3), inputs.record_dense_fasta(27 + 61 * 500, 9, seed=4)
    texts = [inputs.edge_fasta() + x, x + y + inputs.byte_soup(20_000, 5), y]
    counted = [lib().count_fasta(t, k, device=0)["table"].copy() for t in texts]
    want_tables = [oracle.count_fasta(t, k)["table"] for t in texts]
    tables = [HostTable(k, f"t{i}.kin", t) for i, t in enumerate(counted)]
    for op in OPS:
        want = combine_ref.expected(want_tables[:2], want_tables[2:], op, 1, 255, 1, 0)
        assert np.count_nonzero(want) > 100
        monkeypatch.delenv("PK_MERGE_HBM_BUDGET", raising=False)
        whole = extract.combine_tables(tables[:2], tables[2:], op, 1, 255, 1, 0)
        assert whole["n_pieces"] == 1
        monkeypatch.setenv("PK_MERGE_HBM_BUDGET", "200000")  # less the histogram, over three slices and the output's: pieces of 49152 of the 262144 addresses
        out = np.full(4 ** k, SENTINEL, dtype=np.uint8)
        cut = extract.combine_tables(tables[:2], tables[2:], op, 1, 255, 1, 0, out=out)
        assert cut["n_pieces"] == 6 and cut["table"] is out
        for got in (whole, cut):
            assert np.array_equal(got["table"], want) and np.array_equal(got["hist256"], combine_ref.hist256(want))
            assert (got["n_selected"], got["op"], got["n_present"], got["n_absent"], got["min_present"]) == (np.count_nonzero(want), op, 2, 1, 1)
            assert got["kernel_seconds"] > 0


# ------------------------------------------------------------------ 10. CLI, and the loop closed ---
def test_cli_end_to_end_and_back_in(gpu, tmp_path):
    from pykmer_amd.header import Header
    k = 9
    rng = np.random.default_rng(10)
    unit = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 40)])
    kins, tables, texts = [], [], []
    for i in range(3):
        fa = tmp_path / f"s{i}.fa"
        data = bytes(synth.family(i, 20_000)[0])
        assert data.startswith(b">") and data.endswith(b"\n")                  # the records of two files do not join
        if i < 2:
            data += b">repeat\n" + unit * 150 + b"\n"                           # 150 + 150: the pooled count saturates, neither file's does
        fa.write_bytes(data)
        run_py("indexer.py", str(fa), f"s{i}", str(k), cwd=str(tmp_path))
        kins.append(f"{fa}.{k:02d}.kin")
        tables.append(oracle.count_fasta(data, k)["table"])
        texts.append(data)
    raw = tables[0].astype(np.int64) + tables[1]
    assert ((raw > 255) & (tables[0] < 255) & (tables[1] < 255)).any() and not (tables[0] == 255).any()
    pooled = np.minimum(255, raw).astype(np.uint8)
    # ---- the pooled table
    proj = str(tmp_path / "proj")
    argv = ["extract.py", proj, "--present", kins[0], kins[1], "--min-present", "1", "--table", "sum"]
    r = run_py(*argv, cwd=str(tmp_path))
    kin = f"{proj}.{k:02d}.kin"
    assert f"{np.count_nonzero(pooled):,d} k-mers selected" in r.stdout and r.stdout.rstrip().endswith(f"table {kin} (sum)")
    got = np.fromfile(kin, dtype=np.uint8)
    assert np.array_equal(got, pooled) and np.array_equal(got, combine_ref.expected(tables[:2], [], "sum", 1, 255, 1, 0))
    assert np.array_equal(got, oracle.count_fasta(texts[0] + texts[1], k)["table"])
    assert not os.path.exists(proj + ".kmx") and not os.path.exists(proj + ".kmx.txt") and not list(tmp_path.glob("*.tmp"))
    with open(proj + ".kmx.json") as fh:
        meta = json.load(fh)
    assert meta["table"] == "sum" and meta["table_file"] == kin and meta["n_selected"] == np.count_nonzero(pooled)
    assert [d["index_file"] for d in meta["data"]] == kins[:2] and [d["role"] for d in meta["data"]] == ["present", "present"]
    header = Header(kin, index_file=kin)
    header.check_data_index()                                 # recomputes the statistics with pk_table_stats and compares
    assert header.num_kmers == int(pooled.sum(dtype=np.uint64)) == header.vals_sum and header.vals_max == 255
    sources = [Header(f, index_file=f) for f in kins[:2]]
    assert header.chromosomes == [[f"present:{h.project_name}", h.num_kmers] for h in sources] and sources[0].num_kmers > 0
    # ---- and back in: merged, queried against, extracted from
    run_py("merger.py", str(tmp_path / "m"), kin, kins[2], cwd=str(tmp_path))
    assert np.array_equal(np.load(str(tmp_path / "m.001-255.kma"))["matrix"], oracle.gram([pooled, tables[2]]))
    run_py("query.py", str(tmp_path / "q"), str(tmp_path / "s2.fa"), kin, cwd=str(tmp_path))
    want = query_ref.expected(texts[2], k, [pooled], 1, 255)
    z = np.load(str(tmp_path / "q.kmq"))
    assert np.array_equal(z["hits"], want["hits"]) and np.array_equal(z["depth"], want["depth"]) and want["hits"].sum() > 0
    run_py("extract.py", str(tmp_path / "again"), "--present", kin, "--absent", kins[2], cwd=str(tmp_path))
    want_addr, want_counts = extract_ref.expected([pooled], [tables[2]], 1, 255)
    z = np.load(str(tmp_path / "again.kmx"))
    assert np.array_equal(z["addr"], want_addr) and np.array_equal(z["counts"], want_counts) and want_addr.size > 100
    # ---- refusals
    files = [kin, kin + ".json", proj + ".kmx.json"]
    before = [open(f, "rb").read() for f in files]
    r = run_py(*argv, cwd=str(tmp_path), status=1)              # a second run refuses to overwrite
    assert r.returncode == 1 and "error:" in r.stderr and "already exists" in r.stderr
    assert before == [open(f, "rb").read() for f in files]
    r = run_py("-m", "pykmer_amd.extract", str(tmp_path / "twice"), "--present", kins[0], "--absent", kins[0], "--table", "max", cwd=ROOT, status=1)
    assert r.returncode == 1 and "named twice" in r.stderr
    listing = sorted(p.name for p in tmp_path.iterdir())
    r = run_py("extract.py", str(tmp_path / "none"), "--present", kins[0], "--min-count", "255", "--max-count", "255", "--table", "max",
             cwd=str(tmp_path), status=1)
    assert r.returncode == 1 and "error:" in r.stderr and "no k-mer is selected" in r.stderr and "255-255" in r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == listing
