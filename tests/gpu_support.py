"""What the GPU tests share: tables staged in HBM, the feed loop, one pass through a QueryIndexer, the project's scripts as
child processes, and the comparators that more than one test file uses.  Mechanisms only: what a test expects stays in the
test.  This module is not rewritten by pytest, so every assert here carries its own message."""
import functools
import os
import subprocess
import sys

import numpy as np

import fastq_ref
import oracle
import query_ref
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5


def lib():
    from pykmer_amd import _lib
    return _lib


# ------------------------------------------------------------------ device memory ------------------
class Device:
    """Host tables staged in HBM: .bufs and .ptrs.  Freed on exit from the `with`, and when an upload raises; without a
    `with` the buffers belong to whoever takes .bufs (query.Staged frees them)."""

    def __init__(self, tables, min_bytes=0):
        self.bufs = []
        try:
            for t in tables:
                self.bufs.append(lib().DeviceBuffer(max(min_bytes, t.size), 0))
                self.bufs[-1].upload(t)
        except BaseException:
            self.free()
            raise
        self.ptrs = [b.ptr for b in self.bufs]

    def free(self):
        for b in self.bufs:
            b.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


class SentinelOut:
    """Output buffers in HBM, one attribute per keyword (its size in bytes), every byte the sentinel."""

    def __init__(self, **sizes):
        self._bufs = []
        for name, n in sizes.items():
            b = lib().DeviceBuffer(n, 0)
            b.upload(np.full(b.n, SENTINEL, dtype=np.uint8))
            setattr(self, name, b)
            self._bufs.append(b)

    def untouched(self):
        return all(bool((b.download() == SENTINEL).all()) for b in self._bufs)

    def free(self):
        for b in self._bufs:
            b.free()


class HostTable:
    """What the staging loop needs of a Header, backed by a host array."""

    def __init__(self, k, name, table):
        self.kmer_len, self.index_file, self.data_size, self.table = k, name, 4 ** k, table

    def read_table_slice(self, lo, hi, threads=None):
        return self.table[lo:hi]


@functools.lru_cache(maxsize=None)
def tables(k: int, n: int, seed: int):
    return tuple(query_ref.random_tables(k, n, seed))


# ------------------------------------------------------------------ feeding and reading out --------
def feed(q, text, cuts=None):
    """The text in the pieces between the increasing offsets `cuts` (empty pieces are skipped), whole without cuts."""
    buf = np.frombuffer(text, dtype=np.uint8)
    pos = 0
    for c in list(cuts or []) + [len(text)]:
        if c > pos:
            q.feed(buf[pos:c])
            pos = c


def stream(q, text, *, bins=None, coords=False, spectrum=False, pairs=False, cover=False, cuts=None, bins_last=False, reset=True):
    """One pass through a QueryIndexer whose tables are set: the setters, the feeds, finish(), what was switched on, a
    reset.  bins_last: set_bins after the other setters.  Without bins the rows of spectrum and pairs are the records."""
    if bins is not None and not bins_last:
        q.set_bins(bins)
    for on, setter in ((coords, "set_coords"), (spectrum, "set_spectrum"), (pairs, "set_pairs"), (cover, "set_cover")):
        if on:
            getattr(q, setter)(True)
    if bins is not None and bins_last:
        q.set_bins(bins)
    feed(q, text, cuts)
    fin = q.finish()
    n = fin["n_records"]
    recs = q.records(n)
    out = {"fin": fin, "records": recs, "n_valid": recs["n_valid_kmers"].astype(np.uint64)}
    rows = n
    if cover:
        bits, out["n_bases"] = q.cover(len(text))
        out["bits"] = bits.copy()
    elif bins is None:
        hits, depth = q.results(n)
        out.update(hits=hits.copy(), depth=depth.copy())
    else:
        hits, depth, first = q.bin_results(n)
        rows = int(first[-1])
        out.update(bin_hits=hits.copy(), bin_depth=depth.copy(), bin_first=first.copy())
    if coords:
        start, end = q.bin_coords()
        out.update(bin_start=start.copy(), bin_end=end.copy(), coords_s=q.timings()["coords_s"])
    if spectrum:
        out["spectrum"] = q.spectrum(rows).copy()
    if pairs:
        out["shared"] = q.pairs(rows).copy()
    if reset:
        q.reset()
    return out


def by_row(got):
    """`got` of stream() with the tallies of its rows under "hits" and "depth", binned or not."""
    if "bin_hits" in got:
        got["hits"], got["depth"] = got.pop("bin_hits"), got.pop("bin_depth")
    return got


def query(text, k, ptrs, mn=1, mx=255, fmt="fasta", cuts=None):
    """A plain stream through a QueryIndexer of its own; finish()'s histogram of a query is all zero."""
    with lib().QueryIndexer(k, device=0, fmt=fmt) as q:
        q.set_tables(ptrs, mn, mx)
        got = stream(q, text, cuts=cuts, reset=False)
    assert not got["fin"]["hist256"].any(), ("hist256", np.flatnonzero(got["fin"]["hist256"])[:5])
    return got


def _sums(rows, first):
    """Per-record sums of the rows, by a loop (not the function under test)."""
    out = np.zeros((first.size - 1, rows.shape[1]), dtype=np.uint64)
    for r in range(first.size - 1):
        out[r] = rows[int(first[r]):int(first[r + 1])].sum(axis=0, dtype=np.uint64)
    return out


def binned(q, text, W, cuts=None):
    """One binned stream through `q` (tables set), then the same text unbinned through the same indexer: the per-record
    sums of the rows equal the unbinned tallies and bin_first[R] is the row count.  The result holds both."""
    got = stream(q, text, bins=W, cuts=cuts)                 # the reset switches the bins off again
    plain = stream(q, text)
    for key in ("n_records", "num_kmers"):
        assert plain["fin"][key] == got["fin"][key], (key, plain["fin"][key], got["fin"][key])
    first, R = got["bin_first"], plain["fin"]["n_records"]
    assert first.dtype == np.uint64 and first.shape == (R + 1,) and int(first[0]) == 0, ("bin_first", first.dtype, first.shape, first[:1])
    assert int(first[-1]) == got["bin_hits"].shape[0] == got["bin_depth"].shape[0], ("rows", first[-1], got["bin_hits"].shape, got["bin_depth"].shape)
    for rows, key in (("bin_hits", "hits"), ("bin_depth", "depth")):
        sums = _sums(got[rows], first)
        assert np.array_equal(sums, plain[key]), (rows, np.argwhere(sums != plain[key])[:5])
        got[key] = plain[key]
    return got


def _differ(a, b):
    return np.argwhere(a != b)[:5] if a.shape == b.shape else (a.shape, b.shape)


def _same_records(got, want):
    assert got["fin"]["n_records"] == len(want["records"]), ("n_records", got["fin"]["n_records"], len(want["records"]))
    assert got["fin"]["num_kmers"] == int(want["n_valid"].sum()), ("num_kmers", got["fin"]["num_kmers"], int(want["n_valid"].sum()))
    for field, key in (("n_valid_kmers", "n_valid"), ("seq_len", "seq_len")):
        assert np.array_equal(got["records"][field], want[key]), (key, _differ(got["records"][field], want[key]))


def _same_arrays(got, want, keys):
    for key in keys:
        assert got[key].dtype == np.uint64 and got[key].shape == want[key].shape, (key, got[key].dtype, got[key].shape, want[key].shape)
        assert np.array_equal(got[key], want[key]), (key, np.argwhere(got[key] != want[key])[:5], got[key][:8], want[key][:8])


def same(got, want):
    """A plain result of query() or stream() against query_ref.expected."""
    _same_records(got, want)
    _same_arrays(got, want, ("hits", "depth"))
    over = got["hits"] > want["n_valid"][:, None]
    assert not over.any(), ("hits above n_valid", np.argwhere(over)[:5])


def same_bins(got, want):
    """A result of binned() against query_bins_ref.expected."""
    _same_records(got, want)
    _same_arrays(got, want, ("bin_first", "bin_hits", "bin_depth", "hits", "depth"))


def same_coords(got, want):
    """A result of stream(bins=W, coords=True) against query_coords_ref.expected."""
    _same_records(got, want)
    _same_arrays(got, want, ("bin_first", "bin_hits", "bin_depth", "bin_start", "bin_end"))
    assert got["coords_s"] > 0 or want["bin_first"][-1] == 0, ("coords_s", got["coords_s"])


def _option_left_the_rest(got, plain, want, binned):
    """A stream with an option on against the same stream with it off, and the record fields against the yardstick."""
    for key in ("hits", "depth", "n_valid") + (("bin_first",) if binned else ()):
        assert np.array_equal(got[key], plain[key]), (key, _differ(got[key], plain[key]))
    assert np.array_equal(got["n_valid"], want["n_valid"]), ("n_valid", _differ(got["n_valid"], want["n_valid"]))
    assert got["fin"]["num_kmers"] == int(want["n_valid"].sum()), ("num_kmers", got["fin"]["num_kmers"], int(want["n_valid"].sum()))
    if binned:
        assert np.array_equal(got["bin_first"], want["bin_first"]), ("bin_first", _differ(got["bin_first"], want["bin_first"]))


def checked_spectrum(q, text, window, want, W=None, cuts=None, bins_last=False):
    """A stream with the spectrum on and one with it off through `q` (tables set with `window`): the identities, the
    unchanged tallies, and the spectrum against query_spectrum_ref.expected."""
    import query_spectrum_ref
    got = by_row(stream(q, text, bins=W, spectrum=True, cuts=cuts, bins_last=bins_last))
    _option_left_the_rest(got, by_row(stream(q, text, bins=W)), want, W is not None)
    query_spectrum_ref.check_identities(got["spectrum"], want["row_windows"], got["hits"], got["depth"], *window)
    assert got["spectrum"].shape == want["spectrum"].shape, ("spectrum", got["spectrum"].shape, want["spectrum"].shape)
    assert np.array_equal(got["spectrum"], want["spectrum"]), ("spectrum", np.argwhere(got["spectrum"] != want["spectrum"])[:5])
    return got


def checked_pairs(q, text, want, W=None, cuts=None, bins_last=False):
    """A stream with the pairs on and one with them off through `q` (tables set with the window of `want`): the unchanged
    tallies, the bound, and hits and shared against query_pairs_ref.expected."""
    import query_pairs_ref
    got = by_row(stream(q, text, bins=W, pairs=True, cuts=cuts, bins_last=bins_last))
    _option_left_the_rest(got, by_row(stream(q, text, bins=W)), want, W is not None)
    assert np.array_equal(got["hits"], want["hits"]), ("hits", _differ(got["hits"], want["hits"]))
    assert got["shared"].dtype == np.uint64 and got["shared"].shape == want["shared"].shape, ("shared", got["shared"].dtype, got["shared"].shape, want["shared"].shape)
    assert np.array_equal(got["shared"], want["shared"]), ("shared", np.argwhere(got["shared"] != want["shared"])[:5])
    query_pairs_ref.check_identities(got["shared"], got["hits"])
    return got


# ------------------------------------------------------------------ the indexer against the oracle -
def check_against_oracle(gpu, data, k):
    """count_fasta of the library against the oracle's: totals, records, table and histogram."""
    got = gpu.count_fasta(data, k)
    want = oracle.count_fasta(data, k)
    for key in ("num_kmers", "total_bp"):
        assert got[key] == want[key], (key, got[key], want[key])
    assert len(got["records"]) == len(want["records"]), ("records", len(got["records"]), len(want["records"]))
    for f in ("name_off", "name_len", "seq_len", "n_valid_kmers"):
        assert np.array_equal(got["records"][f], want["records"][f]), (f, _differ(got["records"][f], want["records"][f]))
    assert np.array_equal(got["table"], want["table"]), ("table", _differ(got["table"], want["table"]))
    hist, _ = oracle.table_stats(want["table"])
    assert np.array_equal(got["hist256"][1:], hist), ("hist256", _differ(got["hist256"][1:], hist))
    assert int(got["hist256"].sum()) == 4 ** k, ("hist256 sum", int(got["hist256"].sum()))
    return got


def count_fastq(fq, k, cuts=None, n_slices=1, slice_index=0):
    """FASTQ through one indexer, fed whole or in the given pieces; table, totals, records, stats."""
    with lib().Indexer(k, device=0, fmt="fastq", slice_index=slice_index, n_slices=n_slices) as ix:
        feed(ix, fq, cuts)
        fin = ix.finish()
        fin["records"] = ix.records(fin["n_records"])
        fin["stats"] = ix.fastq_stats()
        fin["table"] = ix.table_to_host() if k <= 15 else None
        return fin


def record_names(text, recs):
    return [(text[int(r["name_off"]):int(r["name_off"]) + int(r["name_len"])], int(r["seq_len"]), int(r["n_valid_kmers"])) for r in recs]


def check_fastq_against_oracle(got, fq, k):
    """A result of count_fastq against the oracle's count of the FASTA text that the FASTQ stands for."""
    fa = fastq_ref.fastq_to_fasta(fq)
    want = oracle.count_fasta(fa, k)
    for key in ("num_kmers", "total_bp"):
        assert got[key] == want[key], (key, got[key], want[key])
    assert np.array_equal(got["table"], want["table"]), ("table", _differ(got["table"], want["table"]))
    hist, _ = oracle.table_stats(want["table"])
    assert np.array_equal(got["hist256"][1:], hist), ("hist256", _differ(got["hist256"][1:], hist))
    w = want["records"]
    assert got["n_records"] == len(w), ("n_records", got["n_records"], len(w))
    a, b = record_names(fq, got["records"]), record_names(fa, w)          # names sliced from the FASTQ equal those of the FASTA
    assert a == b, ("records", [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:5])
    assert got["stats"] == fastq_ref.stats(fq), ("stats", got["stats"], fastq_ref.stats(fq))


def accumulate_windows(gpu, tables, windows):
    """Host tables -> device buffers -> ONE pk_gram_device_accumulate_windows call -> W x N x N."""
    N, n = len(tables), tables[0].size
    bufs = [gpu.DeviceBuffer(n, 0) for _ in range(N)]
    acc = gpu.DeviceBuffer(len(windows) * N * N * 8, 0)
    try:
        for b, t in zip(bufs, tables):
            b.upload(t)
        acc.zero()
        gpu.gram_device_accumulate_windows([b.ptr for b in bufs], n, acc.ptr, windows)
        return acc.download().view(np.uint64).reshape(len(windows), N, N)
    finally:
        for b in bufs + [acc]:
            b.free()


# ------------------------------------------------------------------ child processes ----------------
def run_py(script, *argv, cwd=None, status=0, timeout=600, env=None):
    """A script of the repository root (or "-m", module) in a child python: the CompletedProcess, its exit status checked."""
    first = os.path.join(ROOT, script) if script.endswith(".py") else script
    r = subprocess.run([sys.executable, first, *argv], cwd=cwd, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == status, (r.returncode, r.stdout[-2000:] + r.stderr[-2000:])
    return r


def env_without_ranks(**more):
    """The environment without a launcher's WORLD_SIZE, RANK and LOCAL_RANK."""
    env = dict(os.environ, **more)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(v, None)
    return env


def index_cli(tmp_path, names, k, n_bases=20_000):
    """synth.family(i) as <name>.fa for every name, indexed by indexer.py in tmp_path: (.kin paths, the oracle's tables)."""
    kins, tabs = [], []
    for i, name in enumerate(names):
        fa = tmp_path / f"{name}.fa"
        data = bytes(synth.family(i, n_bases)[0])
        fa.write_bytes(data)
        run_py("indexer.py", str(fa), name, str(k), cwd=str(tmp_path))
        kins.append(f"{fa}.{k:02d}.kin")
        tabs.append(oracle.count_fasta(data, k)["table"])
    return kins, tabs


def family_kins(tmp_path, manifest, tag="G7_k7_n13_default"):
    """The inputs of a merger golden, indexed by indexer.py at k = 7: the .kin paths."""
    import inputs
    kins = []
    for i, spec in enumerate(manifest["merger"][tag]["inputs"]):
        fa = tmp_path / f"s{i:02d}.fa"
        fa.write_bytes(inputs.make_input(spec))
        run_py("indexer.py", str(fa), f"s{i}", "7", cwd=str(tmp_path))
        kins.append(f"{fa}.07.kin")
    return kins


def env_with_root():
    """The environment with the repository root in front of PYTHONPATH, for `-m pykmer_amd.<tool>` in another directory."""
    return dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
