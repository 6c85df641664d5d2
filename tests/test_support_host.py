"""CPU: the loops and comparators that the GPU tests share (gpu_support), against a fake query indexer that records every
call and answers from the yardsticks.  The comparators are shown to pass on equal input and to raise on one differing
element, with the key in the message: gpu_support is not rewritten by pytest."""
import numpy as np
import pytest

import fastq_ref
import gpu_support as gs
import mask_ref
import oracle
import query_bins_ref
import query_coords_ref
import query_pairs_ref
import query_ref
import query_spectrum_ref

K, WINDOW = 3, (2, 254)
TEXT = b">a\nACGTTGCAAGGTNACGTACGT\n>empty\n\n>b\nAC\n>c\nGGGTTTACGTAAAACCC\nACGT\n"
TABLES = query_ref.random_tables(K, 3, seed=5)
RECORDS = np.dtype([("seq_len", "<u8"), ("n_valid_kmers", "<u8")])


class FakeQuery:
    """The calls of a QueryIndexer in `calls`; the answers from the yardsticks of the text fed so far.  `tamper`: the name
    of an answer whose first element is off by one."""

    def __init__(self, tamper=None):
        self.calls, self.tamper, self.fed, self.W = [], tamper, b"", None

    def _answer(self, name, array):
        array = array.copy()
        if name == self.tamper:
            array.flat[0] += 1
        return array

    def feed(self, buf):
        self.calls.append(("feed", bytes(buf)))
        self.fed += bytes(buf)

    def set_bins(self, W):
        self.calls.append(("set_bins", W))
        self.W = W

    def __getattr__(self, name):                             # set_coords, set_spectrum, set_pairs, set_cover
        if not name.startswith("set_"):
            raise AttributeError(name)
        return lambda on: self.calls.append((name, on))

    def finish(self):
        self.calls.append(("finish",))
        self.plain = query_ref.expected(self.fed, K, TABLES, *WINDOW)
        return {"n_records": len(self.plain["records"]), "num_kmers": int(self.plain["n_valid"].sum()), "hist256": np.zeros(256, dtype=np.uint64)}

    def records(self, n):
        self.calls.append(("records", n))
        recs = np.zeros(n, dtype=RECORDS)
        recs["seq_len"], recs["n_valid_kmers"] = self.plain["seq_len"], self.plain["n_valid"]
        return recs

    def results(self, n):
        self.calls.append(("results", n))
        return self._answer("hits", self.plain["hits"]), self._answer("depth", self.plain["depth"])

    def bin_results(self, n):
        self.calls.append(("bin_results", n))
        want = query_bins_ref.expected(self.fed, K, TABLES, *WINDOW, self.W)
        return tuple(self._answer(key, want[key]) for key in ("bin_hits", "bin_depth", "bin_first"))

    def bin_coords(self):
        self.calls.append(("bin_coords",))
        want = query_coords_ref.expected(self.fed, K, TABLES, *WINDOW, self.W)
        return self._answer("bin_start", want["bin_start"]), self._answer("bin_end", want["bin_end"])

    def timings(self):
        return {"coords_s": 0.5}

    def spectrum(self, rows):
        self.calls.append(("spectrum", rows))
        return self._answer("spectrum", query_spectrum_ref.expected(self.fed, K, TABLES, self.W)["spectrum"])

    def pairs(self, rows):
        self.calls.append(("pairs", rows))
        return self._answer("shared", query_pairs_ref.expected(self.fed, K, TABLES, *WINDOW, W=self.W)["shared"])

    def cover(self, cap):
        self.calls.append(("cover", cap))
        want = mask_ref.expected(self.fed, K, TABLES, *WINDOW)
        return want["bits"], want["n_bases"]

    def reset(self):
        self.calls.append(("reset",))
        self.fed, self.W = b"", None


# ------------------------------------------------------------------ feed ---------------------------
def test_feed_sends_the_slices_between_increasing_cuts_and_skips_empty_ones():
    q = FakeQuery()
    gs.feed(q, TEXT, [0, 5, 5, 6, 40, len(TEXT)])             # a cut at 0, a repeated cut, a one-byte piece, a cut at the end
    assert q.calls == [("feed", TEXT[:5]), ("feed", TEXT[5:6]), ("feed", TEXT[6:40]), ("feed", TEXT[40:])]
    for cuts in (None, [], [0], [len(TEXT)]):
        q = FakeQuery()
        gs.feed(q, TEXT, cuts)
        assert q.calls == [("feed", TEXT)], cuts
    q = FakeQuery()
    gs.feed(q, np.frombuffer(TEXT, dtype=np.uint8), [7])      # an array is fed like the bytes it holds
    assert q.calls == [("feed", TEXT[:7]), ("feed", TEXT[7:])]
    q = FakeQuery()
    gs.feed(q, b"")
    assert q.calls == []


# ------------------------------------------------------------------ stream -------------------------
def test_stream_sets_the_options_in_both_orders():
    for bins_last, order in ((False, ["set_bins", "set_spectrum", "set_pairs"]), (True, ["set_spectrum", "set_pairs", "set_bins"])):
        q = FakeQuery()
        gs.stream(q, TEXT, bins=4, spectrum=True, pairs=True, bins_last=bins_last)
        n_set = len(order)
        assert [c[0] for c in q.calls[:n_set]] == order and q.calls[n_set][0] == "feed", bins_last
        assert ("set_bins", 4) in q.calls and ("set_spectrum", True) in q.calls
    q = FakeQuery()
    gs.stream(q, TEXT, bins=4, coords=True)
    assert q.calls[:3] == [("set_bins", 4), ("set_coords", True), ("feed", TEXT)]
    q = FakeQuery()
    gs.stream(q, TEXT)                                       # nothing switched on: no setter is called
    assert q.calls[0] == ("feed", TEXT) and not [c for c in q.calls if c[0].startswith("set_")]


def test_stream_reads_rows_by_bins_or_records_and_resets_last():
    want = query_bins_ref.expected(TEXT, K, TABLES, *WINDOW, 4)
    R, B = len(want["records"]), int(want["bin_first"][-1])
    assert B > R == 4
    q = FakeQuery()
    got = gs.stream(q, TEXT, bins=4, spectrum=True, pairs=True, cuts=[9])
    assert [c for c in q.calls if c[0] in ("spectrum", "pairs", "bin_results", "results")] == [("bin_results", R), ("spectrum", B), ("pairs", B)]
    assert q.calls[-1] == ("reset",) and q.calls.count(("reset",)) == 1
    assert [c[0] for c in q.calls[:6]] == ["set_bins", "set_spectrum", "set_pairs", "feed", "feed", "finish"]       # three setters, two feeds
    assert sorted(got) == ["bin_depth", "bin_first", "bin_hits", "fin", "n_valid", "records", "shared", "spectrum"]
    assert got["spectrum"].shape[0] == got["shared"].shape[0] == B and np.array_equal(got["bin_first"], want["bin_first"])
    q = FakeQuery()
    got = gs.stream(q, TEXT, spectrum=True, pairs=True)
    assert [c for c in q.calls if c[0] in ("spectrum", "pairs", "bin_results", "results")] == [("results", R), ("spectrum", R), ("pairs", R)]
    assert q.calls[-1] == ("reset",)
    assert sorted(got) == ["depth", "fin", "hits", "n_valid", "records", "shared", "spectrum"]
    assert got["n_valid"].dtype == np.uint64 and np.array_equal(got["n_valid"], want["n_valid"])
    q = FakeQuery()
    got = gs.stream(q, TEXT, bins=4, coords=True)
    assert sorted(got) == ["bin_depth", "bin_end", "bin_first", "bin_hits", "bin_start", "coords_s", "fin", "n_valid", "records"]
    q = FakeQuery()
    got = gs.stream(q, TEXT, cover=True, reset=False)
    assert ("reset",) not in q.calls and q.calls[-1] == ("cover", len(TEXT)) and ("results", R) not in q.calls
    assert sorted(got) == ["bits", "fin", "n_bases", "n_valid", "records"]
    rows = gs.by_row(gs.stream(FakeQuery(), TEXT, bins=4))
    assert np.array_equal(rows["hits"], want["bin_hits"]) and np.array_equal(rows["depth"], want["bin_depth"]) and "bin_hits" not in rows


# ------------------------------------------------------------------ the comparators ----------------
def _raises_on_one_element(compare, got, want, keys):
    """`compare` passes on `got`, and raises naming the key when one element of got[key] is off by one."""
    compare(got, want)
    for key in keys:
        off = dict(got, **{key: got[key].copy()})
        off[key].flat[off[key].size // 2] += 1
        with pytest.raises(AssertionError, match=key):
            compare(off, want)


def test_same_plain_binned_and_coords():
    _raises_on_one_element(gs.same, gs.stream(FakeQuery(), TEXT), query_ref.expected(TEXT, K, TABLES, *WINDOW), ("hits", "depth"))
    _raises_on_one_element(gs.same_bins, gs.binned(FakeQuery(), TEXT, 4), query_bins_ref.expected(TEXT, K, TABLES, *WINDOW, 4),
                           ("bin_first", "bin_hits", "bin_depth", "hits", "depth"))
    _raises_on_one_element(gs.same_coords, gs.stream(FakeQuery(), TEXT, bins=4, coords=True), query_coords_ref.expected(TEXT, K, TABLES, *WINDOW, 4),
                           ("bin_first", "bin_hits", "bin_depth", "bin_start", "bin_end"))
    want = query_ref.expected(TEXT, K, TABLES, *WINDOW)
    for field, key in (("seq_len", "seq_len"), ("n_valid_kmers", "n_valid")):       # the record fields, in all three
        got = gs.stream(FakeQuery(), TEXT)
        got["records"][field][1] += 1
        with pytest.raises(AssertionError, match=key):
            gs.same(got, want)
    got = gs.stream(FakeQuery(), TEXT)
    got["fin"]["n_records"] += 1
    with pytest.raises(AssertionError, match="n_records"):
        gs.same(got, want)
    got = gs.stream(FakeQuery(), TEXT)
    got["hits"] = got["hits"].astype(np.int64)                # the right numbers in the wrong type
    with pytest.raises(AssertionError, match="hits"):
        gs.same(got, want)


def test_binned_and_the_checked_drivers_raise_on_one_element():
    gs.binned(FakeQuery(), TEXT, 4, cuts=[11])
    for key in ("bin_hits", "bin_depth"):                    # a row that no longer adds up to its record
        with pytest.raises(AssertionError, match=key):
            gs.binned(FakeQuery(tamper=key), TEXT, 4)
    for W in (None, 4):
        spec = query_spectrum_ref.expected(TEXT, K, TABLES, W)
        pairs = query_pairs_ref.expected(TEXT, K, TABLES, *WINDOW, W=W)
        q = FakeQuery()
        got = gs.checked_spectrum(q, TEXT, WINDOW, spec, W=W, cuts=[5], bins_last=True)
        assert np.array_equal(got["spectrum"], spec["spectrum"]) and q.calls[-1] == ("reset",) and q.calls.count(("reset",)) == 2
        got = gs.checked_pairs(FakeQuery(), TEXT, pairs, W=W)
        assert np.array_equal(got["shared"], pairs["shared"])
        with pytest.raises(AssertionError):                  # the identities or the comparison, whichever sees it first
            gs.checked_spectrum(FakeQuery(tamper="spectrum"), TEXT, WINDOW, spec, W=W)
        with pytest.raises(AssertionError, match="shared"):
            gs.checked_pairs(FakeQuery(tamper="shared"), TEXT, pairs, W=W)
        other = dict(pairs, n_valid=pairs["n_valid"] + np.uint64(1))
        with pytest.raises(AssertionError, match="n_valid"):
            gs.checked_pairs(FakeQuery(), TEXT, other, W=W)


class _FakeLibrary:
    """count_fasta of the library, answered by the oracle; `tamper(got)` spoils the answer."""

    def __init__(self, tamper=None):
        self.tamper = tamper

    def count_fasta(self, data, k):
        got = oracle.count_fasta(data, k)
        got["table"], got["records"] = got["table"].copy(), got["records"].copy()
        hist, _ = oracle.table_stats(got["table"])
        got["hist256"] = np.concatenate([[4 ** k - int(hist.sum())], hist]).astype(np.uint64)
        if self.tamper:
            self.tamper(got)
        return got


def test_check_against_oracle_raises_on_one_element():
    got = gs.check_against_oracle(_FakeLibrary(), TEXT, K)
    assert got["num_kmers"] > 0

    def spoil(key, field=None):
        def tamper(got):
            if field:
                got[key][field][1] += 1
            elif isinstance(got[key], np.ndarray):
                got[key][got[key].size // 2] += 1
            else:
                got[key] += 1
        return tamper
    for key, field in (("num_kmers", None), ("total_bp", None), ("table", None), ("hist256", None), ("records", "name_off"), ("records", "seq_len")):
        with pytest.raises(AssertionError, match=field or key):
            gs.check_against_oracle(_FakeLibrary(spoil(key, field)), TEXT, K)


def test_check_fastq_against_oracle_raises_on_one_element():
    fq = b"@r1 first\nACGTACGTAC\n+\nIIIIIIIIII\n@r2\nGGGTTT\n+r2\n!!!!!!\n"
    fa = fastq_ref.fastq_to_fasta(fq)

    def counted():
        want = oracle.count_fasta(fa, K)
        hist, _ = oracle.table_stats(want["table"])
        recs = want["records"].copy()
        recs["name_off"] = [fq.index(b"@r1") + 1, fq.index(b"@r2") + 1]
        return {"num_kmers": want["num_kmers"], "total_bp": want["total_bp"], "table": want["table"].copy(), "n_records": len(recs), "records": recs,
                "hist256": np.concatenate([[0], hist]).astype(np.uint64), "stats": fastq_ref.stats(fq)}
    gs.check_fastq_against_oracle(counted(), fq, K)
    for key in ("num_kmers", "total_bp", "n_records"):
        got = counted()
        got[key] += 1
        with pytest.raises(AssertionError, match=key):
            gs.check_fastq_against_oracle(got, fq, K)
    for key, at in (("table", 7), ("hist256", 1)):
        got = counted()
        got[key][at] += 1
        with pytest.raises(AssertionError, match=key):
            gs.check_fastq_against_oracle(got, fq, K)
    got = counted()
    got["records"]["name_off"][1] += 1                       # another name is sliced from the FASTQ
    with pytest.raises(AssertionError, match="records"):
        gs.check_fastq_against_oracle(got, fq, K)
    got = counted()
    got["stats"] = dict(got["stats"], records=3)
    with pytest.raises(AssertionError, match="stats"):
        gs.check_fastq_against_oracle(got, fq, K)
