"""The one-shot oracle of a text, cut into address slices, and the checks of a sliced indexer against it.

Reference for every case: oracle.kmer_list over the WHOLE text in one piece (oracle/kmer_oracle.c, pinned against the
Python restatement at k = 17, 19, 21 by tests/test_oracle_golden.py), np.unique, saturation at 255, the slice selected by
address // slice size.  Everything is integers; every comparison is exact."""
import numpy as np

import oracle

FIELDS = ("name_off", "name_len", "seq_len", "n_valid_kmers")
GIB = 1 << 30


class Expect:
    def __init__(self, data, k: int, n_slices: int):
        self.data = bytes(data) if not isinstance(data, bytes) else data
        self.k, self.n_slices = k, n_slices
        self.size = 4 ** k // n_slices
        self.kmers, self.want = oracle.kmer_list(self.data, k, records=True)
        self.u, c = np.unique(self.kmers, return_counts=True)
        self.sat = np.minimum(c, 255).astype(np.uint8)
        self.u_slice = (self.u // np.uint64(self.size)).astype(np.int64)

    def slice_of(self, kmer) -> int:
        return int(int(kmer) // self.size)

    def windows_per_slice(self) -> np.ndarray:
        return np.bincount((self.kmers // np.uint64(self.size)).astype(np.int64), minlength=self.n_slices)

    def distinct_per_slice(self) -> np.ndarray:
        return np.bincount(self.u_slice, minlength=self.n_slices)

    def busiest(self, exclude=()) -> int:
        w = self.windows_per_slice()
        w[list(exclude)] = -1
        return int(w.argmax())

    def slice(self, s: int):
        """(addresses inside slice s that must be non-zero, their saturated counts)"""
        sel = self.u_slice == s
        return (self.u[sel] - np.uint64(s * self.size)).astype(np.int64), self.sat[sel]

    def check_totals(self, ix, fin, name_off=None):
        """`name_off`: where the names lie in what the indexer was fed, if that is not the text itself (a FASTQ indexer
        reports offsets into the FASTQ stream, the oracle into the FASTA text it stands for)."""
        want = self.want
        assert fin["num_kmers"] == want["num_kmers"]
        assert fin["total_bp"] == want["total_bp"]
        assert fin["n_records"] == len(want["records"])
        recs = ix.records(fin["n_records"])
        for f in FIELDS:
            assert np.array_equal(recs[f], want["records"][f] if f != "name_off" or name_off is None else name_off), f

    def check(self, ix, s: int, full_table: bool = False, tag=None, name_off=None):
        """finish() of an indexer of slice `s` that was fed the text (in any cuts): totals, every record field, the value
        histogram; full_table: the table bytes at every address that must be non-zero and the number of non-zero bytes."""
        fin = ix.finish()
        self.check_totals(ix, fin, name_off)
        addr, sat = self.slice(s)
        h = fin["hist256"]
        assert int(h.sum()) == self.size, tag
        want_h = np.bincount(sat, minlength=256).astype(np.uint64)
        if not np.array_equal(h[1:], want_h[1:]):
            diff = {int(v): (int(h[v]), int(want_h[v])) for v in np.flatnonzero(h[1:] != want_h[1:]) + 1}
            raise AssertionError(f"{tag}: slice {s} histogram differs from the oracle's, value: (got, want) = {diff}")
        if full_table:
            table = ix.table_to_host()
            assert np.array_equal(table[addr], sat), tag
            assert count_nonzero(table) == addr.size, tag
            del table
        return fin


def count_nonzero(table: np.ndarray) -> int:
    return sum(int(np.count_nonzero(table[o:o + GIB])) for o in range(0, table.size, GIB))


def first_window_at(data: bytes, k: int, cut: int) -> int:
    """Index, in the oracle's text-order k-mer list of `data`, of the first window that does not end in front of byte `cut`:
    the window that crosses the cut and reaches furthest back, or -- right behind a restart -- the one that begins there."""
    return int(oracle.kmer_list(data[:cut], k).size)


def crossing_windows(data: bytes, k: int, cut: int, reach: int = 120_000) -> int:
    """How many valid windows begin in front of byte `cut` and end at or behind it: those an N put there would void."""
    hi = min(len(data), cut + reach)
    return int(oracle.kmer_list(data[:hi], k).size) - int(oracle.kmer_list(data[:cut] + b"N" + data[cut:hi], k).size)


def cover(need: dict) -> dict:
    """need: case -> set of slices, any one of which serves it.  Returns slice -> [cases], greedily few slices."""
    left = dict(need)
    out = {}
    while left:
        tally = {}
        for case, ss in left.items():
            for s in ss:
                tally.setdefault(s, []).append(case)
        best = max(sorted(tally), key=lambda s: len(tally[s]))
        out[best] = tally[best]
        for case in tally[best]:
            del left[case]
    return out


N_SLICES = {17: 2, 19: 16, 21: 256}                      # slices of 2^33 (the 64-bit control) and 2^34 addresses


def seam_slice(exp, cut):
    """The slice of the window that crosses byte `cut` of the text and reaches furthest back (first_window_at)."""
    i = first_window_at(exp.data, exp.k, cut)
    assert i < exp.kmers.size, ("no window crosses byte", cut)
    return exp.slice_of(exp.kmers[i])
