"""pk_unitig and unitigs.py on the GPU at their seams, against tests/unitig_ref.py: tables shorter than one 16-byte load
(k = 1, k = 3), tables with rings alone and rings that carry the row numbering, one builder over several builds, more than
1024 rank workgroups with six-digit rows, slices of the text across the seam of its two parts, and the refusals after a
build.  The inputs are tests/unitig_inputs.py's; test_unitigs_host.py asserts on the reference alone that they hold what
each test here is named for.  Not covered: the step-bound error path (checks 1 to 8), which no table reaches."""
import ctypes

import numpy as np
import pytest

import gpu_support as gs
import unitig_inputs as ui
import unitig_ref as ref
from unitig_support import TOTALS, build_at, read_out, same

pytestmark = pytest.mark.gpu

ROW_KEYS = ("first_addr", "n_kmers", "depth", "circular")


@pytest.fixture(scope="module")
def gpu():
    return gs.lib()


@pytest.fixture(scope="module")
def ring_dev():
    """ring_table() staged once for the module."""
    with gs.Device([ref.table_of(ui.ring_table(), ui.RING_K)]) as dev:
        yield dev.ptrs[0]


def same_named(name, got, want):
    try:
        same(got, want)
    except AssertionError as exc:
        raise AssertionError(f"{name}: {exc}") from exc


def same_builds(name, got, fresh):
    """Two builds of one input, read out by read_out: everything but the timings is equal."""
    for key in TOTALS + ("bytes", "fasta"):
        assert got[key] == fresh[key], (name, key, got[key] if key != "fasta" else len(got[key]), fresh[key] if key != "fasta" else len(fresh[key]))
    for key in ROW_KEYS:
        assert np.array_equal(got[key], fresh[key]), (name, key)


# ------------------------------------------------------------------ A. every small graph -----------
def test_every_table_at_k1(gpu):
    """The 9 tables of 4 addresses under both windows through one builder, each table 4 bytes in a device buffer of its own:
    the cut branch of the 16-byte load and the byte-wise store of the link bytes.  A table without a node builds cleanly."""
    empty = 0
    with gpu.Unitigs(1, device=0) as u:
        for mn, mx in ui.K1_WINDOWS:
            for counts in ui.k1_tables():
                table = ref.table_of(counts, 1)
                assert table.size == 4
                with gs.Device([table]) as dev:
                    assert dev.bufs[0].n == 4
                    got = read_out(u, u.build(dev.ptrs[0], mn, mx))
                want = ref.expected(counts, 1, mn, mx)
                same_named(f"k = 1, bytes {table.tolist()}, window {mn}-{mx}", got, want)
                if want["n_nodes"] == 0:
                    empty += 1
                    assert all(got[key] == 0 for key in TOTALS + ("bytes",)) and got["fasta"] == b"", got
                    assert all(got[key].size == 0 for key in ROW_KEYS)
        assert u.timings()["builds"] == 18
    assert empty >= 2


def test_random_subsets_at_k3(gpu):
    """1500 subsets of the 32 canonical addresses of k = 3 (64 addresses: a quarter of a workgroup's first step), a third of
    them under a second window, through one builder and one device buffer: a byte left over from one subset shows in the
    next.  Self-loops, hairpins, double edges, paths of up to 5 k-mers and rings of 2 and 3 are among them."""
    cases = ui.k3_cases()
    with gs.Device([np.zeros(64, dtype=np.uint8)]) as dev, gpu.Unitigs(3, device=0) as u:
        for name, counts, mn, mx, want in cases:
            dev.bufs[0].upload(ref.table_of(counts, 3))
            same_named(name, read_out(u, u.build(dev.ptrs[0], mn, mx)), want)
        assert u.timings()["builds"] == len(cases)


# ------------------------------------------------------------------ B. rings -----------------------
@pytest.mark.parametrize("build", ui.RING_BUILDS, ids=lambda b: "%d-%d-M%d" % b)
def test_rings_and_their_numbering(gpu, ring_dev, build):
    """1100 rings and 95 paths at k = 11.  The window 1-2 leaves no linear unitig: the linear phase returns with no
    candidate, the rings are rows 0 to 1099 and every decimal width begins in the circular text.  1-255 puts 95 rows in
    front of them.  M = 12 drops 72 rings among the others and numbers the rest anew.  5-5 leaves no loop candidate."""
    mn, mx, M = build
    want = ui.ring_expected(mn, mx, M)
    same(build_at(ring_dev, ui.RING_K, mn, mx, M), want)


@pytest.mark.parametrize("M", [1, 12])
def test_ring_minima_spread_over_the_rank_workgroups(gpu, M):
    """3000 rings and nothing else: one kept candidate per ring among all its nodes, in more than 50 of the rank workgroups
    of 256 loop candidates, and row indices of four digits with row_base = 0."""
    want = ui.wide_ring_expected(M)
    with gs.Device([ref.table_of(ui.wide_ring_table(), ui.RING_K)]) as dev:
        same(build_at(dev.ptrs[0], ui.RING_K, 1, 255, M), want)


# ------------------------------------------------------------------ C. rebuilds --------------------
def test_one_builder_over_many_builds(gpu, ring_dev):
    """One builder over ui.REBUILDS: everything, the rings alone, the paths alone, a window without a node, everything
    again, and an M above every unitig.  Its buffers never shrink, so each build must forget the one before: the totals, the
    rows and the whole text equal the reference's and a fresh builder's."""
    before = (0.0, 0.0, 0.0)
    with gpu.Unitigs(ui.RING_K, device=0) as u:
        for i, (mn, mx, M) in enumerate(ui.REBUILDS):
            name = f"build {i}: window {mn}-{mx}, M = {M}"
            got = read_out(u, u.build(ring_dev, mn, mx, M))
            want = ui.ring_expected(mn, mx, M)
            same_named(name, got, want)
            same_builds(name, got, build_at(ring_dev, ui.RING_K, mn, mx, M))
            if want["n_nodes"] == 0 or len(want["n_kmers"]) == 0:
                assert got["bytes"] == 0 and got["fasta"] == b"" and u.text(0, 0).size == 0 and all(got[key].size == 0 for key in ROW_KEYS), name
            if len(want["n_kmers"]) == 0 and want["n_nodes"]:
                assert got["nodes_short"] == got["n_nodes"] == want["n_nodes"], name
            t = got["timings"]
            now = (t["links_s"], t["paths_s"], t["cycles_s"])
            assert t["builds"] == i + 1 and all(b >= a for a, b in zip(before, now)) and now[0] > before[0], (name, before, now)
            before = now


# ------------------------------------------------------------------ D. more than 1024 rank workgroups
def test_two_scan_rounds_and_six_digit_rows(gpu):
    """293 320 nodes at k = 11 with more than 262 144 + 256 ends: the scans of the rank workgroups' rows and bytes carry
    their running sum into a second round of 1024 entries, and the row indices reach six digits.  With M = 3 about one
    candidate in 25 is kept, so the offsets come from both scans."""
    with gs.Device([ui.dense_table()]) as dev:
        for M in (1, 3):
            same_named(f"M = {M}", build_at(dev.ptrs[0], ui.D_K, 1, 255, M), ui.dense_expected(M))


# ------------------------------------------------------------------ E. slices and refusals ---------
def test_text_slices_across_the_seam_and_refusals(gpu, ring_dev):
    want = ui.ring_expected(1, 255, 1)
    fasta, lin = want["fasta"], ui.linear_bytes(want)
    with gpu.Unitigs(ui.RING_K, device=0) as u:
        got = u.build(ring_dev, 1, 255, 1)
        size, rows = got["bytes"], got["n_linear"] + got["n_circular"]
        assert size == len(fasta) and rows == len(want["n_kmers"]) and 17 < lin < size - 17
        for off in (0, lin - 1, lin, lin + 1, size - 1, size):
            for n in (0, 1, 2, 17):
                if off + n <= size:
                    assert u.text(off, n).tobytes() == fasta[off:off + n], (off, n)
        assert u.text(lin - 9, 17).tobytes() == fasta[lin - 9:lin + 8]
        for off, n in ((size + 1, 0), (size, 1), (lin, size - lin + 1)):
            with pytest.raises(ValueError, match="lie outside"):
                u.text(off, n)
        lib = gpu.load()
        out = [np.full(rows * 8, gs.SENTINEL, dtype=np.uint8).view(np.uint64) for _ in range(3)] + [np.full(rows, gs.SENTINEL, dtype=np.uint8)]
        assert lib.pk_unitig_rows(u._h, *(a.ctypes.data for a in out), rows - 1) == gpu.PK_ERR_RECS_CAP
        assert all(bool((a.view(np.uint8) == gs.SENTINEL).all()) for a in out)
        assert lib.pk_unitig_rows(u._h, None, None, None, None, rows) == gpu.PK_ERR_ARG
        for missing in range(4):
            ptrs = [ctypes.c_void_p(a.ctypes.data) if i != missing else None for i, a in enumerate(out)]
            assert lib.pk_unitig_rows(u._h, *ptrs, rows) == gpu.PK_ERR_ARG
        assert all(bool((a.view(np.uint8) == gs.SENTINEL).all()) for a in out)
        same(read_out(u, got), want)                         # the refusals left the build as it was


@pytest.mark.parametrize("piece", ["1000", "lin", "lin + 1"])
def test_the_text_comes_back_in_slices(gpu, ring_dev, piece, tmp_path, monkeypatch):
    """build_unitigs reads the text in pieces of TEXT_SLICE: pieces of 1000 bytes, and pieces that end at, and one byte
    behind, the seam of the linear and the circular text, give the bytes of the one default piece, returned or written."""
    from pykmer_amd import staging, unitigs
    want = ui.ring_expected(1, 255, 1)
    lin = ui.linear_bytes(want)
    table = staging.ResidentTable(ring_dev, 4 ** ui.RING_K, 4 ** ui.RING_K)
    assert unitigs.TEXT_SLICE > len(want["fasta"])
    whole = unitigs.build_unitigs(table)
    monkeypatch.setattr(unitigs, "TEXT_SLICE", {"1000": 1000, "lin": lin, "lin + 1": lin + 1}[piece])
    assert len(want["fasta"]) > 2 * unitigs.TEXT_SLICE
    got = unitigs.build_unitigs(table)
    assert got["fasta"] == whole["fasta"] == want["fasta"] and got["bytes"] == len(want["fasta"])
    path = tmp_path / "u.fa"
    filed = unitigs.build_unitigs(table, out_file=path)
    assert filed["output"] == str(path) and "fasta" not in filed and path.read_bytes() == want["fasta"]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["u.fa"]
