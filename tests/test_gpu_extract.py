"""GPU: the extract kernels (kmer_extract.hip, pk_extract_device / pk_extract_text) and the host path above them against the
numpy restatement (extract_ref); exact equality everywhere."""
import ctypes
import json

import numpy as np
import pytest

import gpu_support as gs
import extract_ref
import inputs
import oracle
from gpu_support import ROOT, SENTINEL, Device, HostTable, SentinelOut, index_cli, lib, run_py

pytestmark = pytest.mark.gpu


class _Out(SentinelOut):
    """Output arrays of `cap` rows in HBM, filled with a sentinel."""

    def __init__(self, cap, P):
        self.cap, self.P = cap, P
        super().__init__(addr=max(16, cap * 8), counts=max(16, cap * P))

    def rows(self, m):
        return self.addr.download(m * 8).view(np.uint64), self.counts.download(m * self.P).reshape(m, self.P)


def _run(ptrs, P, n, mn, mx, min_present, max_absent, cap, first_addr=0):
    """One pk_extract_device call into fresh sentinel-filled arrays of `cap` rows -> (n_selected, fits, addr, counts, untouched)."""
    out = _Out(cap, P)
    try:
        m, fits, _ = lib().extract_device(ptrs, P, n, first_addr, mn, mx, min_present, max_absent, out.addr.ptr, out.counts.ptr, cap)
        if not fits:
            return m, False, None, None, out.untouched()
        addr, counts = out.rows(m)
        tail_ok = (out.addr.download()[m * 8:] == SENTINEL).all() and (out.counts.download()[m * P:] == SENTINEL).all()
        return m, True, addr, counts, bool(tail_ok)
    finally:
        out.free()


def _check(present, absent, mn, mx, min_present=None, max_absent=0, first_addr=0, n=None):
    P = len(present)
    n = present[0].size if n is None else n
    min_present = P if min_present is None else min_present
    want_addr, want_counts = extract_ref.expected([t[:n] for t in present], [t[:n] for t in absent], mn, mx, min_present, max_absent, first_addr)
    with Device(present + absent, min_bytes=16) as dev:
        m, fits, addr, counts, tail_ok = _run(dev.ptrs, P, n, mn, mx, min_present, max_absent, want_addr.size + 3, first_addr)
    assert m == want_addr.size and fits and tail_ok
    assert np.array_equal(addr, want_addr), np.flatnonzero(addr != want_addr)[:5]
    assert np.array_equal(counts, want_counts), np.argwhere(counts != want_counts)[:5]
    return want_addr.size


# ------------------------------------------------------------------ 1. slice sizes -----------------
@pytest.mark.parametrize("n", [1, 15, 16, 31, 32, 1023, 1024, 2047, 2048, 2049, 4 ** 7, 4 ** 7 + 17])
def test_slice_sizes(gpu, n):
    """The tables are longer than the slice and hold selectable bytes behind it: nothing at or beyond n_slice is read as
    data.  4^7 + 17 addresses are two workgroups, the second one 17 addresses long."""
    tables = extract_ref.mixed_tables(n + 64, 3, seed=n, zero=0.3)
    for t in tables[:2]:
        t[n:] = 100
    tables[2][n:] = 0
    m = _check(tables[:2], tables[2:], 2, 200, n=n)
    assert n < 64 or 0 < m < n


# ------------------------------------------------------------------ 2. selection density -----------
def test_selection_density(gpu):
    n = 4 ** 7 + 17
    hold, none = np.full(n, 5, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    with Device([hold, none, hold], min_bytes=16) as dev:
        m, fits, addr, counts, untouched = _run(dev.ptrs, 2, n, 1, 255, 2, 0, 64)      # present: hold, none -> nothing selected
        assert (m, fits) == (0, True) and addr.size == 0 and untouched
        m, fits, addr, counts, untouched = _run([dev.ptrs[0], dev.ptrs[2]], 1, n, 1, 255, 1, 0, 64)   # absent holds everything
        assert (m, fits) == (0, True) and untouched
    assert _check([hold, hold], [none], 1, 255) == n                                    # everything selected
    for at in (0, n - 1, 4096 + 77):
        one = none.copy()
        one[at] = 200
        rng = np.random.default_rng(at)
        other = rng.integers(1, 256, n).astype(np.uint8)
        with Device([one, other, none], min_bytes=16) as dev:
            m, fits, addr, counts, tail_ok = _run(dev.ptrs, 2, n, 1, 255, 2, 0, 1)
        assert (m, fits, tail_ok) == (1, True, True) and addr.tolist() == [at] and counts.tolist() == [[200, int(other[at])]]


# ------------------------------------------------------------------ 3. large addresses -------------
def test_addresses_beyond_32_bits(gpu):
    tables = extract_ref.mixed_tables(5000, 3, seed=33)
    first = 2 ** 33 + 2048
    want, _ = extract_ref.expected(tables[:2], tables[2:], 2, 200, 1, 0, first)
    assert want[0] >= first and want.dtype == np.uint64
    _check(tables[:2], tables[2:], 2, 200, 1, 0, first_addr=first)


# ------------------------------------------------------------------ 3b. row widths -----------------
@pytest.mark.parametrize("P", [3, 5, 6, 7, 9, 127])
def test_row_widths(gpu, P):
    """Rows of P bytes, P not 1, 2 or a multiple of 4: a tile's byte range [g0, g1) of the count array starts at every
    offset within a dword that P allows, its dwords start in the middle of a row, and rows wrap inside a dword."""
    present, absent, residues = extract_ref.row_width_case(P)
    assert residues == ({0, 2} if P == 6 else {0, 1, 2, 3})
    n = present[0].size
    assert n % extract_ref.TILE == 17 and n > 4 * extract_ref.TILE           # two workgroups or more, the last tile 17 addresses
    m = _check(present, absent, 2, 200, 1, 0)
    assert n // 5 < m < n // 2
    if P == 3:
        _check(present, absent, 2, 200, 1, 0, first_addr=2 ** 33 + 2048)


# ------------------------------------------------------------------ 3c. short ranges ---------------
PER_TILE = [2, 1, 0, 1,  3, 2, 1, 3,  0, 0, 0, 0,  1, 3, 0, 2,  1]    # selected addresses per tile; four tiles are a workgroup


@pytest.mark.parametrize("P", [1, 3])
def test_ranges_inside_one_dword(gpu, P):
    """One, two or three rows per tile: byte ranges shorter than the dword they lie in, and short ranges with an unaligned
    head and tail.  P = 1 gives a range that starts off a dword boundary and ends before the next one; three bytes that
    start off a boundary end at the next one at the earliest, so for P = 3 the range inside one dword ends on it, and only
    P = 3 (nine bytes from three rows) has a whole dword between an unaligned head and an unaligned tail."""
    present, absent, mask = extract_ref.sparse_tiles(PER_TILE, P, seed=20 + P)
    per = np.add.reduceat(mask.astype(np.int64), np.arange(0, mask.size, extract_ref.TILE))
    assert per.tolist() == PER_TILE and mask.size == 16 * extract_ref.TILE + 17
    assert per[2] == 0 and per[1] and per[3]                            # an empty tile inside a workgroup that selects
    assert per[8:12].sum() == 0 and per[4:8].sum() and per[12:16].sum()   # an empty workgroup between two that select
    g0, g1 = extract_ref.tile_ranges(mask, P)
    dword = g0 & ~3
    one_dword = (g1 > g0) & (g0 % 4 != 0) & (g1 <= dword + 4)
    around = (g0 % 4 != 0) & (g1 % 4 != 0) & (((g0 + 3) & ~3) + 4 <= (g1 & ~3))
    if P == 1:
        assert (one_dword & (g1 < dword + 4)).any()
    else:
        assert one_dword.any() and around.any()
    assert _check(present, absent, 1, 255) == sum(PER_TILE)


# ------------------------------------------------------------------ 4. counter edges ---------------
def test_counters_reach_128(gpu):
    n = 4100
    rng = np.random.default_rng(4)
    full = [rng.integers(1, 256, n).astype(np.uint8) for _ in range(128)]
    short = rng.integers(0, 128, n)                          # at odd addresses table short[x] lacks x: 127 hold it
    for x in range(1, n, 2):
        full[short[x]][x] = 0
    assert _check(full, [], 1, 255, 128) == (n + 1) // 2      # p = 128 selected, p = 127 not
    assert _check(full, [], 1, 255, 127) == n
    # P = 1, A = 127, max_absent = 126: q = 126 selected, q = 127 not
    present = [np.full(n, 3, dtype=np.uint8)]
    absent = [t.copy() for t in full[:127]]
    for x in range(n):
        absent[x % 127][x] = 0 if x % 3 else absent[x % 127][x]      # two addresses in three: one absent table lacks x (q = 126)
    q = sum((t >= 1).astype(np.int32) for t in absent)
    assert set(np.unique(q)) >= {126, 127}
    m = _check(present, absent, 1, 255, 1, 126)
    assert m == int((q <= 126).sum()) and 0 < m < n


def test_thresholds_on_random_tables(gpu):
    tables = extract_ref.mixed_tables(4 ** 7 + 17, 32, seed=5, zero=0.6)
    m = _check(tables[:16], tables[16:], 2, 200, 9, 3)
    assert m > 0
    assert _check(tables[:16], tables[16:], 2, 200, 1, 16) > m


# ------------------------------------------------------------------ 5. window edges ----------------
@pytest.mark.parametrize("mn,mx", [(2, 200), (1, 255), (128, 129), (127, 127), (255, 255), (2, 254)])
def test_window_edges(gpu, mn, mx):
    edge = np.array(sorted({max(mn - 1, 0), mn, mx, min(mx + 1, 255), 0, 255, 1, 127, 128}), dtype=np.uint8)
    a = np.repeat(edge, edge.size)                           # every pair of edge values
    b = np.tile(edge, edge.size)
    absent = np.zeros(a.size, dtype=np.uint8)
    absent[::5] = 1                                          # count 1 is held, whatever the window
    absent[1::7] = 255
    _check([a, b], [absent], mn, mx)                         # both in the window, absent nowhere
    m = _check([a, b], [absent], mn, mx, 1, 0)               # min_present < P: rows carry out-of-window bytes as they are
    want_addr, want_counts = extract_ref.expected([a, b], [absent], mn, mx, 1, 0)
    out_of_window = (want_counts < mn) | (want_counts > mx)
    assert m == want_addr.size and out_of_window.any() and not (absent[want_addr.astype(np.int64)] != 0).any()
    _check([a, b], [absent], mn, mx, 2, 1)                   # the absent table tolerated


# ------------------------------------------------------------------ 6. capacity --------------------
def test_capacity(gpu):
    lib = gs.lib()
    tables = extract_ref.mixed_tables(4 ** 7 + 17, 3, seed=6)
    want_addr, want_counts = extract_ref.expected(tables[:2], tables[2:], 2, 200, 1, 0)
    M = want_addr.size
    assert M > 100
    with Device(tables, min_bytes=16) as dev:
        m, fits, _, _, untouched = _run(dev.ptrs, 2, tables[0].size, 2, 200, 1, 0, M - 1)
        assert (m, fits, untouched) == (M, False, True)
        out = _Out(M - 1, 2)
        count = ctypes.c_uint64(0)
        ptrs = (ctypes.c_void_p * 3)(*dev.ptrs)
        rc = lib.load().pk_extract_device(ptrs, 2, 1, tables[0].size, 0, 2, 200, 1, 0, ctypes.c_void_p(out.addr.ptr), ctypes.c_void_p(out.counts.ptr),
                                          M - 1, ctypes.byref(count), 0, None)
        assert rc == lib.PK_ERR_RECS_CAP and count.value == M and out.untouched()
        out.free()
        m, fits, addr, counts, tail_ok = _run(dev.ptrs, 2, tables[0].size, 2, 200, 1, 0, M)
        assert (m, fits, tail_ok) == (M, True, True) and np.array_equal(addr, want_addr) and np.array_equal(counts, want_counts)
        rc = lib.load().pk_extract_device(ptrs, 2, 1, tables[0].size, 0, 2, 200, 1, 0, None, None, 0, ctypes.byref(count), 0, None)
        assert rc == lib.PK_OK and count.value == M          # cap = 0, no arrays: the count alone
        assert lib.extract_device(dev.ptrs, 2, tables[0].size, 0, 2, 200, 1, 0)[0] == M


# ------------------------------------------------------------------ 7. arguments -------------------
def test_bad_arguments_are_refused(gpu):
    lib = gs.lib()
    n = 4096
    t = np.full(n, 3, dtype=np.uint8)
    with Device([t], min_bytes=16) as dev:
        p = dev.ptrs[0]
        out = _Out(16, 1)
        count = ctypes.c_uint64(0)

        def rc(tabs, P, A, mn=1, mx=255, minp=1, maxa=0, addr=out.addr.ptr, counts=out.counts.ptr, cap=16, count_ref=ctypes.byref(count)):
            ptrs = (ctypes.c_void_p * max(1, len(tabs)))(*tabs) if tabs is not None else None
            return lib.load().pk_extract_device(ptrs, P, A, n, 0, mn, mx, minp, maxa, ctypes.c_void_p(addr) if addr else None,
                                                ctypes.c_void_p(counts) if counts else None, cap, count_ref, 0, None)
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
        assert rc([p], 1, 0, addr=None) == lib.PK_ERR_ARG and rc([p], 1, 0, counts=None) == lib.PK_ERR_ARG
        assert rc([p], 1, 0, count_ref=None) == lib.PK_ERR_ARG
        assert out.untouched()
        assert rc([p], 1, 0) == lib.PK_ERR_RECS_CAP and count.value == n and out.untouched()   # and a good call still works
        for k in (0, 33):
            assert lib.load().pk_extract_text(ctypes.c_void_p(out.addr.ptr), 1, k, ctypes.c_void_p(out.counts.ptr), 0) == lib.PK_ERR_ARG
        assert lib.load().pk_extract_text(None, 1, 9, ctypes.c_void_p(out.counts.ptr), 0) == lib.PK_ERR_ARG
        assert lib.load().pk_extract_text(ctypes.c_void_p(out.addr.ptr), 1, 9, None, 0) == lib.PK_ERR_ARG
        out.free()


# ------------------------------------------------------------------ 8. text ------------------------
@pytest.mark.parametrize("k", list(range(1, 32, 2)) + [32])
def test_text(gpu, k):
    """Every odd k and the largest one: a thread writes 16 bytes and a line is k + 1, so where lines end inside a thread's
    bytes differs with (k + 1) mod 16; from k = 18 on the addresses need more than 35 bits.  1000 lines are two
    workgroups or more from k = 5 on."""
    lib = gs.lib()
    rng = np.random.default_rng(k)
    for m in (1, 2, 7, 1000):
        addr = rng.integers(0, 4 ** k, m, dtype=np.uint64)
        addr[0] = 0
        addr[-1] = 4 ** k - 1
        a = lib.DeviceBuffer(m * 8, 0)
        a.upload(addr.view(np.uint8))
        text = lib.DeviceBuffer((m * (k + 1) + 15) // 16 * 16 + 16, 0)
        text.upload(np.full(text.n, SENTINEL, dtype=np.uint8))
        lib.extract_text(a.ptr, m, k, text.ptr)
        got = text.download()
        assert got[:m * (k + 1)].tobytes() == extract_ref.decode(addr, k).tobytes()
        assert (got[m * (k + 1):] == SENTINEL).all()
        lib.extract_text(a.ptr, 0, k, text.ptr)               # m = 0: a no-op
        lib.extract_text(None, 0, k, None)
        assert np.array_equal(text.download(), got)
        a.free()
        text.free()
    if k == 9:
        assert extract_ref.decode([5 << 8], 9).tobytes() == b"AAACCAAAA\n"


# ------------------------------------------------------------------ 9. the whole path, small -------
def test_whole_path_under_a_small_budget(gpu, monkeypatch):
    from pykmer_amd import extract
    k = 9
    x, y = inputs.record_dense_fasta(27 + 61 * 1000, 9, seed=3), inputs.record_dense_fasta(27 + 61 * 500, 9, seed=4)
    texts = [inputs.edge_fasta() + x, x + y + inputs.byte_soup(20_000, 5), y]
    counted = [lib().count_fasta(t, k, device=0)["table"].copy() for t in texts]
    want_tables = [oracle.count_fasta(t, k)["table"] for t in texts]
    tables = [HostTable(k, f"t{i}.kin", t) for i, t in enumerate(counted)]
    want = extract_ref.expected(want_tables[:2], want_tables[2:], 1, 255, 2, 0)
    assert want[0].size > 100
    monkeypatch.delenv("PK_MERGE_HBM_BUDGET", raising=False)
    whole = extract.extract_kmers(tables[:2], tables[2:], 1, 255, text=True)
    assert whole["n_pieces"] == 1
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", "200000")      # less 2048 output rows of 20 bytes, over three tables: slices of 51200 of the 262144 addresses
    cut = extract.extract_kmers(tables[:2], tables[2:], 1, 255, text=True, initial_rows=16)
    assert cut["n_pieces"] == 6 and cut["n_calls"] > 6
    for got in (whole, cut):
        assert np.array_equal(got["addr"], want[0]) and np.array_equal(got["counts"], want[1])
        assert got["text"].tobytes() == extract_ref.decode(want[0], k).tobytes()
        assert (got["n_selected"], got["n_present"], got["n_absent"], got["min_present"], got["max_absent"]) == (want[0].size, 2, 1, 2, 0)
    loose = extract.extract_kmers(tables[:2], tables[2:], 2, 255, min_present=1, max_absent=1, hbm_budget=1)   # output floor: halving
    want = extract_ref.expected(want_tables[:2], want_tables[2:], 2, 255, 1, 1)
    assert np.array_equal(loose["addr"], want[0]) and np.array_equal(loose["counts"], want[1])


# ------------------------------------------------------------------ 10. one full-size case ---------
def test_full_size_table(gpu):
    """k = 15: 2^30 addresses, 65536 workgroups (64 rounds of the scan), ranks far beyond one workgroup's."""
    lib = gs.lib()
    k, n = 15, 4 ** 15
    pool_a = np.zeros(64, dtype=np.uint8)
    pool_a[[3, 17, 18, 40, 63]] = [2, 200, 201, 1, 77]
    pool_b = np.zeros(64, dtype=np.uint8)
    pool_b[[17, 41]] = [1, 9]
    a, b = np.tile(pool_a, n // 64), np.tile(pool_b, n // 64)
    rng = np.random.default_rng(15)
    a[rng.integers(0, n, 20_000)] = 50                       # breaks the period: ranks drift along the table
    b[rng.integers(0, n, 20_000)] = 1
    mask = (a >= 2) & (a <= 200) & (b == 0)
    M = int(np.count_nonzero(mask))
    want_addr = np.flatnonzero(mask).astype(np.uint64)
    assert 2 ** 25 < M < 2 ** 26
    with Device([a, b], min_bytes=16) as dev:
        addr, counts = lib.DeviceBuffer(M * 8, 0), lib.DeviceBuffer((M + 15) // 16 * 16, 0)
        m, fits, secs = lib.extract_device(dev.ptrs, 1, n, 0, 2, 200, 1, 0, addr.ptr, counts.ptr, M)
        assert (m, fits) == (M, True) and secs > 0
        ranks = np.concatenate([np.arange(1000), np.arange(M - 1000, M), np.sort(rng.integers(0, M, 1000))])
        for r in ranks[::50]:                                 # 60 probes of 50 consecutive ranks
            r = int(min(r, M - 50))
            got_addr = addr.download(50 * 8, r * 8).view(np.uint64)
            got_counts = counts.download(50, r)
            assert np.array_equal(got_addr, want_addr[r:r + 50]), r
            assert np.array_equal(got_counts, a[want_addr[r:r + 50].astype(np.int64)]), r
        head, tail = addr.download(8000, 0).view(np.uint64), addr.download(8000, (M - 1000) * 8).view(np.uint64)
        assert np.array_equal(head, want_addr[:1000]) and np.array_equal(tail, want_addr[-1000:])
        assert np.array_equal(counts.download(1000, 0), a[want_addr[:1000].astype(np.int64)])
        assert np.array_equal(counts.download(1000, M - 1000), a[want_addr[-1000:].astype(np.int64)])
        addr.free()
        counts.free()


def test_scan_second_round_of_one_workgroup(gpu):
    """1025 workgroups: k_extract_scan takes their counts 1024 at a time, the second round holds one, and its rank hangs on
    the first round's total.  The last workgroup is 17 addresses long; addresses on both sides of the seam are selected."""
    wg = 4 * extract_ref.TILE                                # addresses per workgroup
    n = 1024 * wg + 17
    rng = np.random.default_rng(1025)
    a, b = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    at = rng.integers(0, n, 40_000)
    a[at] = rng.integers(1, 256, at.size)
    a[[0, 1024 * wg - 1, 1024 * wg, n - 1]] = 100
    b[rng.integers(1, 1024 * wg - 1, 20_000)] = 1
    want_addr, _ = extract_ref.expected([a], [b], 2, 200)
    assert want_addr[0] == 0 and (want_addr >= 1024 * wg).sum() >= 2 and want_addr[-1] == n - 1 and 10_000 < want_addr.size < 40_000
    _check([a], [b], 2, 200)


# ------------------------------------------------------------------ 11. CLI ------------------------
def test_cli_end_to_end(gpu, tmp_path):
    k = 9
    kins, tables = index_cli(tmp_path, ("s0", "s1", "s2"), k)
    want = extract_ref.expected(tables[:2], tables[2:], 1, 250, 1, 0)
    proj = str(tmp_path / "proj")
    argv = ["extract.py", proj, "--present", kins[0], kins[1], "--absent", kins[2], "--max-count", "250", "--min-present", "1",
            "--kmers"]
    r = run_py(*argv, cwd=str(tmp_path))
    assert f"{want[0].size:,d} k-mers selected" in r.stdout
    z = np.load(proj + ".kmx")
    assert np.array_equal(z["addr"], want[0]) and np.array_equal(z["counts"], want[1]) and z["addr"].dtype == np.uint64
    assert (int(z["kmer_len"]), int(z["min_count"]), int(z["max_count"]), int(z["min_present"]), int(z["max_absent"])) == (k, 1, 250, 1, 0)
    with open(proj + ".kmx.json") as fh:
        meta = json.load(fh)
    assert meta["n_selected"] == want[0].size and [d["role"] for d in meta["data"]] == ["present", "present", "absent"]
    assert [d["index_file"] for d in meta["data"]] == kins
    lines = open(proj + ".kmx.txt", "rb").read().split(b"\n")
    assert len(lines) == want[0].size + 1 and lines[-1] == b"" and all(len(ln) == k and set(ln) <= set(b"ACGT") for ln in lines[:-1])
    assert b"\n".join(lines) == extract_ref.decode(want[0], k).tobytes()
    before = [open(proj + ext, "rb").read() for ext in (".kmx", ".kmx.json", ".kmx.txt")]
    r = run_py(*argv, cwd=str(tmp_path), status=1)              # a second run refuses to overwrite
    assert r.returncode == 1 and "error:" in r.stderr and "already exists" in r.stderr
    assert before == [open(proj + ext, "rb").read() for ext in (".kmx", ".kmx.json", ".kmx.txt")]
    r = run_py("-m", "pykmer_amd.extract", str(tmp_path / "twice"), "--present", kins[0], "--absent", kins[0], cwd=ROOT, status=1)
    assert "named twice" in r.stderr

