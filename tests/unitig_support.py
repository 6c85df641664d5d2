"""What the GPU tests of the unitig builder share: one build read out whole, and its comparison with a result of
tests/unitig_ref.py -- the totals, the four row arrays and the FASTA bytes, for equality.  This module is not rewritten by
pytest, so every assert here carries its own message."""
import numpy as np

import gpu_support as gs
import unitig_ref as ref

TOTALS = ("n_nodes", "n_branching", "n_linear", "n_circular", "n_short", "nodes_short", "longest_kmers")


def read_out(u, got):
    """The totals `got` of a build of the builder u, with its rows, its text and its timings."""
    got.update(u.rows())
    got["fasta"] = u.text().tobytes()
    assert u.text(0, 0).size == 0, ("text(0, 0)", u.text(0, 0).size)
    if got["bytes"] >= 3:                                    # any slice of the text
        assert u.text(1, got["bytes"] - 2).tobytes() == got["fasta"][1:-1], "text(1, bytes - 2)"
    got["timings"] = u.timings()
    return got


def build_at(ptr, k, mn=1, mx=255, M=1):
    """pk_unitig_build on the table at ptr: totals, rows, fasta, timings."""
    with gs.lib().Unitigs(k, device=0) as u:
        return read_out(u, u.build(ptr, mn, mx, M))


def same(got, want):
    for key in TOTALS:
        assert got[key] == want[key], (key, got[key], want[key])
    assert got["bytes"] == len(want["fasta"]), ("bytes", got["bytes"], len(want["fasta"]))
    for key in ("first_addr", "n_kmers", "depth", "circular"):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (key, got[key].dtype, got[key].shape, want[key].shape)
        assert np.array_equal(got[key], want[key]), (key, np.flatnonzero(got[key] != want[key])[:5], got[key][:8], want[key][:8])
    if got["fasta"] != want["fasta"]:
        at = next(i for i, (a, b) in enumerate(zip(got["fasta"], want["fasta"])) if a != b)
        raise AssertionError(("fasta", at, got["fasta"][max(0, at - 40):at + 40], want["fasta"][max(0, at - 40):at + 40]))


def check(counts, k, mn=1, mx=255, M=1, want=None):
    want = want or ref.expected(counts, k, mn, mx, M)
    with gs.Device([ref.table_of(counts, k)]) as dev:
        got = build_at(dev.ptrs[0], k, mn, mx, M)
    same(got, want)
    return got, want
