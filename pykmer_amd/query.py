"""Query host side: a FASTA / FASTQ file and N `.kin[.bgz]` tables in, per-record k-mer hits out.

For every record r of the query (file order; records without a valid window included) and every table t:
    hits[r][t]  = number of valid windows of r whose canonical k-mer has min_count <= T_t[a] <= max_count
    depth[r][t] = sum of T_t[a] over those windows (depth / hits = mean count of the matched k-mers)
The reference has no such tool (its README stops at the distance matrix); the text is parsed exactly as the indexer parses
it (pk_query_* in include/pykmer_hip.h: the indexer's structure pass and squeeze, then lookups instead of counting).

The tables are staged in HBM the way the merger stages them (raw `.kin` mapped, `.kin.bgz` inflated block-parallel).  When
they do not all fit the HBM budget they are staged in groups and the query is streamed once per group: the columns are
independent, so the results concatenate.  One device (PK_DEVICE).

With `bin_windows` = W the same tallies are also kept along each record, in bins of W valid windows (pk_query_set_bins):
record r with m valid windows j = 0 .. m-1 has ceil(m / W) bins, bin b holding the windows b*W <= j < min((b+1)*W, m); the
rows are ordered by record, then by bin, and bin_first[r] is record r's first row (bin_first[R] = the number of rows).

With `coords` every row also gets its place on the record in bases (pk_query_set_coords): bin_start = the position of the
first base of the row's first window, bin_end = one past the last base of its last window, positions counted within the
record as seq_len counts them (0-based; every sequence character, valid or not, and the blanks inside a sequence line).

With `spectrum` the same lookup also tallies, per row (record, or bin) and table, how many valid windows have each table
count (pk_query_set_spectrum): spectrum[row][t][c], c = 0 .. 255, zeros (absent k-mers) included and independent of the
count window.  Hits and depth of any window, the median and every quantile of a row's k-mer counts follow from it
(pykmer_amd.qspectrum re-windows a written `.kmh` without tables or a GPU).

With `pairs` the same lookup also tallies, per row and pair of tables i < j, the valid windows that lie in the count window
of both (pk_query_set_pairs): shared[row][p], p the index of (i, j) in spectrum.pair_list(N).  With hits as the diagonal a
row is a `.kma`-shaped matrix of its own: local Jaccard distances and trees along a record (pykmer_amd.qpairs).  A pair
needs both tables in one lookup: at most 16 tables, staged as one group.
"""
import argparse
import os
import sys
from pathlib import Path
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib, staging
from .header import Header
from .indexer import _Input, _mark, qual_threshold
from .merger import DEFAULT_THREADS
from .spectrum import pair_list
from .output import atomic_write, write_json
from .tables import EXTS, MAX_KMER_LEN, common_kmer_len, lean_headers, name_of as _name_of, table_entry   # noqa: F401

MAX_PAIR_TABLES = 16                # pk_query_set_pairs: the tables of a pair meet in one lookup launch (QUERY_MAX_TABLES)
WORKSPACE_RESERVE = 4 << 30         # of the free HBM, kept for the feed's workspace when the budget is taken from mem_info


def load_header(path, device: int = 0) -> Header:
    """The Header of one `.kin[.bgz]`; what the Header refuses (no metadata, an even kmer_len) is reported with the file's name."""
    kins = str(path)
    if not kins.endswith(EXTS[:2]):
        raise ValueError(f"all tables must be .{Header.IND_EXT}[.{Header.COMP_EXT}] files: {kins}")
    if not os.path.exists(kins):
        raise ValueError(f"table file does not exist: {kins}")
    try:
        return Header(kins, index_file=kins, device=device)
    except AssertionError as exc:
        raise ValueError(f"{kins}: not a usable k-mer table (kmer_len must be positive and odd): {exc}") from exc


def validate(tables: Sequence, min_count: int, max_count: int) -> int:
    """The checks that need no device; returns the common kmer_len.  `tables`: Headers (or anything with kmer_len)."""
    if not 1 <= min_count <= max_count <= 255:
        raise ValueError(f"the count window must satisfy 1 <= min <= max <= 255, got {min_count}-{max_count}")
    if len(tables) < 1:
        raise ValueError("a query needs at least one table")
    return common_kmer_len(tables, "query")


def validate_bins(bin_windows) -> int:
    """W of `--bin` / `bin_windows`: an integer >= 1 (a bool or a float is none)."""
    if isinstance(bin_windows, (bool, np.bool_)) or not isinstance(bin_windows, (int, np.integer)):
        raise ValueError(f"the bin size must be an integer number of windows, got {bin_windows!r}")
    if not 1 <= int(bin_windows) < 2 ** 64:
        raise ValueError(f"the bin size must be at least 1 window (and below 2^64), got {int(bin_windows)}")
    return int(bin_windows)


def record_sums(rows: np.ndarray, bin_first: np.ndarray) -> np.ndarray:
    """(R, N) sums of the (B, N) `rows` over each record's rows [bin_first[r], bin_first[r + 1]); a record without a row
    sums to zero (np.add.reduceat would give it the next record's first row)."""
    rows = np.asarray(rows, dtype=np.uint64)
    first = np.asarray(bin_first, dtype=np.int64)
    assert rows.ndim == 2 and first.ndim == 1 and first.size >= 1 and first[0] == 0 and first[-1] == rows.shape[0] \
        and np.all(np.diff(first) >= 0), "bin_first does not describe the rows"
    cum = np.zeros((rows.shape[0] + 1, rows.shape[1]), dtype=np.uint64)
    np.cumsum(rows, axis=0, out=cum[1:])
    return cum[first[1:]] - cum[first[:-1]]


def spectrum_record_sums(rows: np.ndarray, bin_first: np.ndarray) -> np.ndarray:
    """record_sums for (B, N, 256) spectra: the (R, N, 256) sums over each record's rows."""
    rows = np.asarray(rows, dtype=np.uint64)
    assert rows.ndim == 3
    width = rows.shape[1] * rows.shape[2]                   # (spelled out: a query without a window has no row to infer it from)
    return record_sums(rows.reshape(rows.shape[0], width), bin_first).reshape((len(bin_first) - 1,) + rows.shape[1:])


def table_groups(n_tables: int, table_bytes: int, budget: int) -> List[Tuple[int, int]]:
    """[lo, hi) index ranges of the tables staged together: as many as fit `budget` bytes, at least one."""
    per = max(1, int(budget) // max(1, int(table_bytes)))
    return [(lo, min(n_tables, lo + per)) for lo in range(0, n_tables, per)]


class Staged:
    """Device pointers of one group of tables and the buffers behind them (none for tables that were resident already)."""

    def __init__(self, ptrs, bufs=()):
        self.ptrs, self.bufs = list(ptrs), list(bufs)

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


class _Piece:
    """The buffers of the piece a suspended staging.staged_pieces holds: free() closes the generator, which frees them."""

    def __init__(self, pieces):
        self.free = pieces.close


def stage_tables(tables: Sequence, device: int, threads: int = DEFAULT_THREADS) -> Staged:
    """Whole tables into HBM, `threads` at a time: the one piece [0, 4^k) of staging.staged_pieces, which stays suspended
    behind the Staged until its free(); a staging.ResidentTable is used where it lies."""
    pieces = staging.staged_pieces(tables, [(0, tables[0].data_size)], device, threads)
    ptrs, _, _ = next(pieces)
    return Staged(ptrs, [_Piece(pieces)])


def as_headers(tables: Sequence, device: int = 0) -> list:
    """`tables` with every `.kin[.bgz]` path turned into its Header; Headers and resident tables stay as they are."""
    return [load_header(t, device) if isinstance(t, (str, os.PathLike)) else t for t in tables]


def set_options(bin_windows=None, coords=False, spectrum=False, pairs=False, **more) -> dict:
    """The option keywords that query, query_records and `run` hand on: only those that are set (`more`: the caller's own)."""
    given = {} if bin_windows is None else {"bin_windows": bin_windows}
    given.update({name: True for name, on in (("coords", coords), ("spectrum", spectrum), ("pairs", pairs)) if on})
    return {**given, **more}


def plan_groups(tables: Sequence, kmer_len: int, device: int = 0, hbm_budget: int = None) -> List[Tuple[int, int]]:
    """The [lo, hi) ranges of `tables` staged together: one group when they are resident, else what the HBM budget holds
    beside the feed's workspace (table_groups)."""
    if all(hasattr(t, "device_slice") for t in tables):
        return [(0, len(tables))]                            # resident already: nothing to fit
    return table_groups(len(tables), 4 ** kmer_len, staging.hbm_budget(device, hbm_budget, workspace=WORKSPACE_RESERVE))


def stream_groups(query_file: str, tables: Sequence, kmer_len: int, groups, min_count: int, max_count: int, run, join, device: int = 0,
                  threads: int = DEFAULT_THREADS, stage=None, **extra) -> dict:
    """The group loop of every tool that streams a query against staged tables: per group of `groups` (plan_groups) stage,
    `run(query_file, kmer_len, ptrs, min_count, max_count, device, first, **extra)`, free.  `join(result, part)` -> result says
    how a group's part joins the result of the groups before (None for the first group); the records of a later part must be
    those of the first.  The result gains kmer_len, min_count, max_count, n_groups and lookup_s, the sum over the groups.
    `stage(tables, device)` -> Staged defaults to stage_tables."""
    stage = stage or (lambda group, dev: stage_tables(group, dev, threads))
    result, lookup_s = None, 0.0
    for g, (lo, hi) in enumerate(groups):
        staged = stage(tables[lo:hi], device)
        _mark(f"tables {lo}..{hi - 1} staged")
        try:
            part = run(query_file, kmer_len, staged.ptrs, min_count, max_count, device, g == 0, **extra)
        finally:
            staged.free()
        _mark(f"query streamed against tables {lo}..{hi - 1}")
        lookup_s += float(part.get("timings", {}).get("lookup_s", 0.0))
        assert result is None or (np.array_equal(part["n_valid"], result["n_valid"]) and np.array_equal(part["seq_len"], result["seq_len"])), \
            "query changed between table groups"
        result = join(result, part)
    result.update(kmer_len=kmer_len, min_count=min_count, max_count=max_count, n_groups=len(groups), lookup_s=lookup_s)
    return result


def run_query(query_file: str, kmer_len: int, ptrs, min_count: int, max_count: int, device: int = 0, first: bool = True,
              bin_windows: int = None, coords: bool = False, min_qual_byte: int = 0, spectrum: bool = False, pairs: bool = False) -> dict:
    """Streams the query once against the staged tables `ptrs`.  `first`: also fetch the record names (later groups of the
    same query only add columns).  `bin_windows`: tally per bin (bin_hits, bin_depth, bin_first); the per-record arrays
    are then the sums of each record's rows.  `coords`: also bin_start, bin_end -- on the `first` stream only, they do
    not depend on the tables.  `min_qual_byte`: a FASTQ query's bases below this quality byte count as N (qual_threshold).
    `spectrum`: also the count spectra, `spectrum` (R, N, 256) and, binned, `bin_spectrum` (B, N, 256).
    `pairs`: also the shared windows of every pair of tables, `shared` (R, P) and, binned, `bin_shared` (B, P)."""
    coords = bool(coords) and first
    src = _Input(query_file, keep=first, quiet=not first)
    binned = {}
    with _lib.QueryIndexer(kmer_len, device=device, fmt=src.fmt, min_qual_byte=min_qual_byte) as q:
        q.set_tables(ptrs, min_count, max_count)
        if bin_windows is not None:
            q.set_bins(bin_windows)
            if coords:
                q.set_coords(True)
        if spectrum:
            q.set_spectrum(True)
        if pairs:
            q.set_pairs(True)
        for piece in src.pieces():
            q.feed(piece)
        fin = q.finish()
        recs = q.records(fin["n_records"])
        if bin_windows is not None:
            bin_hits, bin_depth, bin_first = q.bin_results(fin["n_records"])
            hits, depth = record_sums(bin_hits, bin_first), record_sums(bin_depth, bin_first)
            binned = {"bin_hits": bin_hits.copy(), "bin_depth": bin_depth.copy(), "bin_first": bin_first}
            if coords:
                bin_start, bin_end = q.bin_coords()
                binned.update(bin_start=bin_start.copy(), bin_end=bin_end.copy())
            if spectrum:
                binned["bin_spectrum"] = q.spectrum(int(bin_first[-1]))
                binned["spectrum"] = spectrum_record_sums(binned["bin_spectrum"], bin_first)
            if pairs:
                binned["bin_shared"] = q.pairs(int(bin_first[-1])).copy()
                binned["shared"] = record_sums(binned["bin_shared"], bin_first)
        else:
            hits, depth = q.results(fin["n_records"])
            if spectrum:
                binned["spectrum"] = q.spectrum(fin["n_records"])
            if pairs:
                binned["shared"] = q.pairs(fin["n_records"]).copy()
        timings = q.timings()
        masked = {"masked": q.fastq_masked()} if min_qual_byte else {}
    out = {"seq_len": recs["seq_len"].astype(np.uint64), "n_valid": recs["n_valid_kmers"].astype(np.uint64), "hits": hits.copy(),
           "depth": depth.copy(), "num_kmers": fin["num_kmers"], "total_bp": fin["total_bp"], "timings": timings, **binned, **masked}
    if first:
        out["names"] = [nm.decode("utf-8", "replace") for nm in src.names(recs)]
    return out


def query_records(query_file: str, tables: Sequence, min_count: int = 1, max_count: int = 255, device: int = 0, hbm_budget: int = None,
                  threads: int = DEFAULT_THREADS, stage=None, run=None, bin_windows: int = None, coords: bool = False, min_qual: int = 0, qual_offset: int = 33,
                  spectrum: bool = False, pairs: bool = False) -> dict:
    """Per-record hits of `query_file` (FASTA or FASTQ by its name; plain, gzip or BGZF) against `tables`: Headers,
    merger.ResidentTables or `.kin[.bgz]` paths.  Returns dict(names, seq_len (R,), n_valid (R,), hits (R, N), depth (R, N),
    kmer_len, ...), all integer arrays uint64, rows in file order, columns in the order of `tables`.

    `hbm_budget` (bytes; default PK_MERGE_HBM_BUDGET, else 80 % of the free HBM less the feed's workspace) bounds the tables
    staged beside each other; more are staged group after group, the query streamed once per group.
    `stage(tables, device)` -> Staged and `run(query_file, kmer_len, ptrs, min_count, max_count, device, first)` -> dict
    default to stage_tables / run_query (the CPU-only tests substitute both).

    `bin_windows` = W >= 1 adds bin_hits, bin_depth (B, N) and bin_first (R + 1,), uint64: the same tallies per bin of W
    valid windows along each record (the module's docstring); hits / depth are then the sums over each record's rows, from
    the same single lookup.  `run` receives bin_windows by keyword, and only when it is set.

    `coords` = True (with `bin_windows`; ValueError without) adds bin_start and bin_end (B,), uint64: the base positions
    within its record of the first base of every row's first window and one past the last base of its last (the module's
    docstring).  They are computed while the first table group is streamed.  `run` receives coords like bin_windows.

    `min_qual` = Q > 0 (a FASTQ query only; ValueError otherwise): bases whose quality byte is below Q + qual_offset count
    as N (README "Base quality"); the result gains `masked`, their number.  `run` receives min_qual_byte by keyword, and
    only when it is set.

    `spectrum` = True adds `spectrum` (R, N, 256) uint64, spectrum[r][t][c] = the valid windows of record r whose count in
    table t is c (0 = absent; the count window plays no part), and `median` (R, N) uint8, the lower median of those counts
    (qspectrum.median_from_spectrum).  With `bin_windows` also `bin_spectrum` (B, N, 256) and `bin_median` (B, N), and
    `spectrum` is the sum over each record's rows.  `run` receives spectrum=True by keyword, and only when it is set.

    `pairs` = True adds `shared` (R, P) uint64, P = N (N - 1) / 2, shared[r][p] = the valid windows of record r whose count
    lies in the count window in both tables of pair p, and `pairs` (P, 2) int32, the tables (i, j), i < j, of every p in
    row-major order (spectrum.pair_list).  With `bin_windows` also `bin_shared` (B, P), and `shared` is the sum over each
    record's rows.  The tables of a pair meet in one lookup: ValueError for more than 16 tables, for tables that do not fit
    the budget as one group, and together with `spectrum`.  `run` receives pairs=True by keyword, and only when it is set."""
    if pairs and spectrum:
        raise ValueError("pairs and spectrum are tallied in separate runs (the spectrum takes the tables one after the other): "
                         "--pairs and --spectrum do not go together")
    if bin_windows is not None:
        bin_windows = validate_bins(bin_windows)
    if coords and bin_windows is None:
        raise ValueError("coordinates are those of bins: coords needs bin_windows (--coords needs --bin W)")
    extra = set_options(bin_windows, coords, spectrum, pairs,
                        **({"min_qual_byte": qual_threshold(str(query_file), min_qual, qual_offset)} if min_qual else {}))
    tables = as_headers(tables, device)
    kmer_len = validate(tables, min_count, max_count)
    if pairs and len(tables) > MAX_PAIR_TABLES:
        raise ValueError(f"pairs take at most {MAX_PAIR_TABLES} tables, all in one lookup; got {len(tables)}")
    groups = plan_groups(tables, kmer_len, device, hbm_budget)
    if pairs and len(groups) > 1:
        raise ValueError(f"pairs need all {len(tables)} tables of {4 ** kmer_len:,d} bytes staged together, and the HBM budget holds "
                         f"{groups[0][1]} at a time: take fewer tables or a larger budget (PK_MERGE_HBM_BUDGET)")
    binned = bin_windows is not None
    columns = ["hits", "depth"] + (["bin_hits", "bin_depth"] if binned else []) + ((["spectrum", "bin_spectrum"] if binned else ["spectrum"]) if spectrum else [])
    coords_s = 0.0

    def join(result, part):
        """A later group's columns behind those of the groups before; the first group's part is the result."""
        nonlocal coords_s
        if result is None:
            if coords:
                coords_s, lookup_s = (float(part.get("timings", {}).get(key, 0.0)) for key in ("coords_s", "lookup_s"))
                _mark(f"coordinate kernels: {coords_s:.6f} s of HIP-event time (lookup kernels: {lookup_s:.6f} s)")
            return part
        if binned:
            assert np.array_equal(part["bin_first"], result["bin_first"]), "bins changed between table groups"
        for key in columns:
            result[key] = np.concatenate([result[key], part[key]], axis=1)
        return result

    result = stream_groups(query_file, tables, kmer_len, groups, min_count, max_count, run or run_query, join, device, threads, stage, **extra)
    if bin_windows is not None:
        result["bin_windows"] = bin_windows
    if spectrum:
        from .qspectrum import median_from_spectrum
        result["median"] = median_from_spectrum(result["spectrum"])
        if bin_windows is not None:
            result["bin_median"] = median_from_spectrum(result["bin_spectrum"])
    if pairs:
        result["pairs"] = pair_list(len(tables))
        assert result["shared"].shape == (len(result["n_valid"]), len(result["pairs"]))
    if coords:
        assert result["bin_start"].shape == result["bin_end"].shape == (int(result["bin_first"][-1]),)
        result["coords_s"] = coords_s
    if min_qual:
        result.update(min_qual=int(min_qual), qual_offset=int(qual_offset))
    return result


def _qual_keys(result: dict) -> dict:
    """min_qual and qual_offset of the `.kmq.json` / `.kmb.json`: only when the query ran with --min-qual."""
    return {"min_qual": int(result["min_qual"]), "qual_offset": int(result["qual_offset"])} if result.get("min_qual") else {}


def _write_rows(paths, project_name: str, result: dict, query_file: str, data: list, heads: List[str], cells: str, values: dict,
                binned: bool, coords: bool = False, window: bool = True, json_more: dict = None, npz_more: dict = None) -> None:
    """The three files of one kind of row values, `paths` = (npz, json, tsv), each through `.tmp` + rename, in that order
    json, tsv, npz.  `values`: npz name -> (array, dtype, shape of one row); the rows are the records, `binned` the bins of
    result["bin_first"].  The tsv has the leading columns record, seq_len, n_valid (binned: record, bin, first_window,
    n_windows, and with `coords` and a result that holds them start, end), then under `heads` the row of values[cells].
    The json has the common keys (`window`: the count window among them), binned bin_windows and n_bins, "coords" with the
    coordinates, `json_more` and _qual_keys; the npz the values, n_valid, seq_len, kmer_len, the count window, binned
    bin_first and bin_windows, the coordinates, and `npz_more`."""
    npz, meta, tsv = paths
    n_valid, seq_len = (np.ascontiguousarray(result[key], dtype=np.uint64) for key in ("n_valid", "seq_len"))
    names = [n.strip() for n in result["names"]]
    assert n_valid.shape == seq_len.shape == (len(names),)
    counts = {"min_count": int(result["min_count"]), "max_count": int(result["max_count"])} if window else {}
    arrays, more, span, rows = {}, {}, {}, len(names)
    if binned:
        W = int(result["bin_windows"])
        bin_first = np.ascontiguousarray(result["bin_first"], dtype=np.uint64)
        assert bin_first.shape == (len(names) + 1,)
        rows = int(bin_first[-1])
        arrays = {"bin_first": bin_first, "bin_windows": np.uint64(W)}
        more = {"bin_windows": W, "n_bins": rows}
        if coords and "bin_start" in result:
            span = {key: np.ascontiguousarray(result[key], dtype=np.uint64) for key in ("bin_start", "bin_end")}
            assert span["bin_start"].shape == span["bin_end"].shape == (rows,)
            more["coords"] = True
    shapes = {name: (rows,) + tuple(shape) for name, (_, _, shape) in values.items()}
    values = {name: np.ascontiguousarray(a, dtype=dtype) for name, (a, dtype, _) in values.items()}
    assert all(values[name].shape == shapes[name] for name in values)

    def leads():
        """(row, its leading columns), in row order"""
        for r, name in enumerate(names):
            if not binned:
                yield r, [name, str(int(seq_len[r])), str(int(n_valid[r]))]
                continue
            m = int(n_valid[r])
            for b in range(int(bin_first[r + 1]) - int(bin_first[r])):
                at = int(bin_first[r]) + b
                yield at, [name, str(b), str(b * W), str(min(W, m - b * W))] + [str(int(span[key][at])) for key in span]

    output = {"project_name": project_name, "kmer_len": int(result["kmer_len"]), **counts, "query_file": str(query_file), "records": names,
              "data": data, **more, **(json_more or {})}
    output.update(_qual_keys(result))
    write_json(meta, output)
    with atomic_write(tsv, "wt") as fhd:
        lead = ["record", "bin", "first_window", "n_windows"] + (["start", "end"] if span else []) if binned else ["record", "seq_len", "n_valid"]
        fhd.write("\t".join(lead + [str(h) for h in heads]) + "\n")
        for at, lead in leads():
            fhd.write("\t".join(lead + [str(int(v)) for v in values[cells][at]]) + "\n")
    with atomic_write(npz, "wb") as fhd:
        np.savez_compressed(fhd, **values, **(npz_more or {}), n_valid=n_valid, seq_len=seq_len, kmer_len=np.int64(result["kmer_len"]),
                            **{key: np.int64(v) for key, v in counts.items()}, **arrays, **span)


def kmq_paths(project_name: str) -> Tuple[Path, Path, Path]:
    return Path(f"{project_name}.kmq"), Path(f"{project_name}.kmq.json"), Path(f"{project_name}.kmq.tsv")


def write_kmq(project_name: str, result: dict, query_file: str, data: list, columns: List[str]) -> None:
    """`<project>.kmq` (np.savez_compressed), `.kmq.json` and `.kmq.tsv`, each through `.tmp` + rename."""
    row = (len(columns),)
    _write_rows(kmq_paths(project_name), project_name, result, query_file, data, columns, "hits",
                {"hits": (result["hits"], np.uint64, row), "depth": (result["depth"], np.uint64, row)}, binned=False)


def kmb_paths(project_name: str) -> Tuple[Path, Path, Path]:
    return Path(f"{project_name}.kmb"), Path(f"{project_name}.kmb.json"), Path(f"{project_name}.kmb.tsv")


def write_kmb(project_name: str, result: dict, query_file: str, data: list, columns: List[str]) -> None:
    """`<project>.kmb` (np.savez_compressed), `.kmb.json` and `.kmb.tsv`: the binned rows, each file through `.tmp` + rename.
    A result with bin_start / bin_end (coords) adds them to the `.kmb`, `"coords": true` to the json and the columns
    `start` and `end` to the tsv; without them the files hold none of the three."""
    row = (len(columns),)
    _write_rows(kmb_paths(project_name), project_name, result, query_file, data, columns, "hits",
                {"hits": (result["bin_hits"], np.uint64, row), "depth": (result["bin_depth"], np.uint64, row)}, binned=True, coords=True)


def kmh_paths(project_name: str) -> Tuple[Path, Path, Path]:
    return Path(f"{project_name}.kmh"), Path(f"{project_name}.kmh.json"), Path(f"{project_name}.kmh.tsv")


def write_kmh(project_name: str, result: dict, query_file: str, data: list, columns: List[str]) -> None:
    """`<project>.kmh` (np.savez_compressed), `.kmh.json` and `.kmh.tsv`: the count spectra of a result with `spectrum`, each
    file through `.tmp` + rename.  The rows are the records; those of a binned result (bin_spectrum) are its bins, and the
    `.kmh` then holds bin_first and bin_windows and the json bin_windows and n_bins.  The json has the keys of the
    `.kmq.json` but the count window, which the spectra do not depend on; the tsv has the leading columns of the `.kmq.tsv`
    (binned: of the `.kmb.tsv`, without coordinates) and every table's median count."""
    from .qspectrum import median_from_spectrum
    binned = "bin_spectrum" in result
    spec = np.ascontiguousarray(result["bin_spectrum" if binned else "spectrum"], dtype=np.uint64)
    key = "bin_median" if binned else "median"
    median = result[key] if key in result else median_from_spectrum(spec)
    N = len(columns)
    _write_rows(kmh_paths(project_name), project_name, result, query_file, data, columns, "median",
                {"spectrum": (spec, np.uint64, (N, 256)), "median": (median, np.uint8, (N,))}, binned=binned, window=False)


def kmp_paths(project_name: str) -> Tuple[Path, Path, Path]:
    return Path(f"{project_name}.kmp"), Path(f"{project_name}.kmp.json"), Path(f"{project_name}.kmp.tsv")


def write_kmp(project_name: str, result: dict, query_file: str, data: list, columns: List[str]) -> None:
    """`<project>.kmp` (np.savez_compressed), `.kmp.json` and `.kmp.tsv`: the shared windows of a result with `pairs`, each
    file through `.tmp` + rename.  The rows are the records; those of a binned result (bin_shared) are its bins, and the
    files then hold what the `.kmb` files hold besides (bin_first, bin_windows, n_bins; with coordinates bin_start, bin_end,
    "coords", the columns start and end).  The `.kmp` holds the rows' hits next to `shared`: a row's matrix needs no other
    file (pykmer_amd.qpairs).  The json has the keys of the `.kmq.json` and n_pairs; the tsv has the leading columns of the
    `.kmq.tsv` (binned: of the `.kmb.tsv`), then one column `<name_i>|<name_j>` per pair."""
    binned = "bin_shared" in result
    pairs = np.ascontiguousarray(result["pairs"], dtype=np.int32).reshape(-1, 2)
    N = len(columns)
    assert pairs.shape == (N * (N - 1) // 2, 2)
    _write_rows(kmp_paths(project_name), project_name, result, query_file, data, [f"{columns[i]}|{columns[j]}" for i, j in pairs], "shared",
                {"shared": (result["bin_shared" if binned else "shared"], np.uint64, (len(pairs),)),
                 "hits": (result["bin_hits" if binned else "hits"], np.uint64, (N,))},
                binned=binned, coords=True, json_more={"n_pairs": len(pairs)}, npz_more={"pairs": pairs})


def refuse_files(outputs: Sequence[Path], inputs: Sequence) -> None:
    """How query, filter and mask open, behind their own checks: no output is overwritten, and every input is there."""
    for f in outputs:
        if f.exists():
            raise ValueError(f"project output file ({f}) already exists. not overwriting.")
    for f in inputs:
        if not os.path.exists(f):
            raise ValueError(f"query file does not exist: {f}")


def verified_tables(indexes: Sequence, min_count: int, max_count: int, device: int = 0) -> Tuple[list, list]:
    """... and then: the `data` entries of the tables `indexes` (tables.table_entry) and their Headers, validated."""
    data = [table_entry(pos, kin, lambda kin: load_header(kin, device)) for pos, kin in enumerate(indexes)]
    headers = [v["header"] for v in data]
    validate(headers, min_count, max_count)
    _mark("tables verified")
    return data, headers


def query(project_name: str, query_file: str, indexes: List[Path], min_count: int = 1, max_count: int = 255, device: int = 0,
          threads: int = DEFAULT_THREADS, hbm_budget: int = None, bin_windows: int = None, coords: bool = False, min_qual: int = None,
          qual_offset: int = None, spectrum: bool = False, pairs: bool = False) -> dict:
    """The CLI's work: validate, query, write the three files (six with `bin_windows`); returns query_records' result.
    `coords` (with `bin_windows`) adds the rows' base coordinates to the `.kmb` files.  `min_qual` / `qual_offset`
    (--min-qual, --qual-offset; None: not given) mask a FASTQ query's low-quality bases and are recorded in the json files.
    `spectrum` (--spectrum) also writes the three `.kmh` files: the count spectra of the rows (write_kmh).
    `pairs` (--pairs; not with `spectrum`, at most 16 tables in one staged group) also writes the three `.kmp` files: the
    shared windows of every pair of tables per row (write_kmp)."""
    if pairs and spectrum:
        raise ValueError("--pairs and --spectrum do not go together (the spectrum takes the tables one after the other): run them separately")
    qual_threshold(str(query_file), min_qual, qual_offset)
    if bin_windows is not None:
        bin_windows = validate_bins(bin_windows)
    if coords and bin_windows is None:
        raise ValueError("--coords gives the coordinates of bins: it needs --bin W")
    extra = set_options(bin_windows, coords, spectrum, pairs,
                        **({"min_qual": min_qual, "qual_offset": 33 if qual_offset is None else qual_offset} if min_qual else {}))
    refuse_files(kmq_paths(project_name) + (kmb_paths(project_name) if bin_windows is not None else ()) + (kmh_paths(project_name) if spectrum else ())
                 + (kmp_paths(project_name) if pairs else ()), [query_file])
    if len(indexes) < 1:
        raise ValueError("a query needs at least one table")
    if pairs and len(indexes) > MAX_PAIR_TABLES:
        raise ValueError(f"--pairs takes at most {MAX_PAIR_TABLES} tables, all in one lookup; got {len(indexes)}")
    data, headers = verified_tables(indexes, min_count, max_count, device)
    try:
        result = query_records(query_file, headers, min_count, max_count, device=device, hbm_budget=hbm_budget, threads=threads,
                               **extra)
    except _lib.PkError as exc:
        if spectrum and exc.code == _lib.PK_ERR_HIP and "count spectra need" in str(exc):
            raise ValueError(f"{exc}; the spectra of --spectrum do not fit the device") from exc
        if pairs and exc.code == _lib.PK_ERR_HIP and "shared windows need" in str(exc):
            raise ValueError(f"{exc}; the shared windows of --pairs do not fit the device") from exc
        if bin_windows is None or exc.code != _lib.PK_ERR_HIP or "bins of" not in str(exc):
            raise
        raise ValueError(f"{exc}; the rows of --bin {bin_windows} do not fit the device: use a larger --bin") from exc
    columns = [str(h.project_name) for h in headers]
    lean_headers(data)
    write_kmq(project_name, result, query_file, data, columns)
    if bin_windows is not None:
        write_kmb(project_name, result, query_file, data, columns)
    if spectrum:
        write_kmh(project_name, result, query_file, data, columns)
    if pairs:
        write_kmp(project_name, result, query_file, data, columns)
    _mark("files renamed")
    return result


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Per-record k-mer hits of a FASTA/FASTQ file against kmer databases.")
    parser.add_argument("Project_Name", metavar="P", type=str, help="Project name (prefix of the output files)")
    parser.add_argument("Query", metavar="Q", type=str, help="queries.fa|.fq[.gz|.bgz]")
    parser.add_argument("Kmer_N", metavar="K", type=Path, nargs="+", help="List of kin files")
    parser.add_argument("--min-count", type=int, default=1, help="Minimum Kmer Count [1]")
    parser.add_argument("--max-count", type=int, default=255, help="Maximum Kmer Count [255]")
    parser.add_argument("--threads", type=int, default=DEFAULT_THREADS, help=f"Host threads reading / inflating the tables [{DEFAULT_THREADS}]")
    parser.add_argument("--bin", type=int, default=None, metavar="W", dest="bin_windows",
                        help="Also write <P>.kmb[.json|.tsv]: the hits along each record in bins of W valid windows [off]")
    parser.add_argument("--coords", action="store_true",
                        help="With --bin: add every bin's base coordinates within its record (start, end) to the .kmb files [off]")
    parser.add_argument("--spectrum", action="store_true",
                        help="Also write <P>.kmh[.json|.tsv]: per record (with --bin: per bin) and table the count spectrum of its "
                             "k-mers and their median count; python -m pykmer_amd.qspectrum re-windows it [off]")
    parser.add_argument("--pairs", action="store_true",
                        help="Also write <P>.kmp[.json|.tsv]: per record (with --bin: per bin) and pair of tables the k-mers found in "
                             "both; at most 16 tables, not with --spectrum; python -m pykmer_amd.qpairs makes a row's .kma [off]")
    parser.add_argument("--min-qual", type=int, default=None, metavar="Q",
                        help="FASTQ query: bases with a quality below Q count as N [off]")
    parser.add_argument("--qual-offset", type=int, default=None, metavar="O", help="With --min-qual: the quality encoding, 33 or 64 [33]")
    return parser


def main(argv: List[str] = None) -> None:
    args = build_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    try:
        result = query(args.Project_Name, args.Query, args.Kmer_N, min_count=args.min_count, max_count=args.max_count,
                       device=int(os.environ.get("PK_DEVICE", "0")), threads=args.threads,
                       **set_options(args.bin_windows, args.coords, args.spectrum, args.pairs,
                                     **({"min_qual": args.min_qual, "qual_offset": args.qual_offset}
                                        if args.min_qual is not None or args.qual_offset is not None else {})))
    except ValueError as exc:
        print(f"error: {exc}", file=sys.stderr)
        sys.exit(1)
    hits = result["hits"]
    print(f"{len(result['names'])} records, {int(result['n_valid'].sum()):,d} k-mers, {hits.shape[1]} tables, "
          f"{result['n_groups']} table group(s)" + (f", {int(result['bin_first'][-1]):,d} bins" if args.bin_windows is not None else "")
          + (f", {len(result['pairs'])} pairs" if args.pairs else ""))
