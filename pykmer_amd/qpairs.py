"""Shared k-mers per query row: a `.kma`-shaped matrix for every record, or every bin along a record, from ONE lookup.

`query.py P Q K... --pairs` tallies, per row (a record of the query, or a bin of `--bin W`) with the valid windows
a_1 .. a_m and per pair of tables i < j,
    shared[row][p] = #{ j : min <= T_i[a_j] <= max and min <= T_j[a_j] <= max }        uint64, exact
p being the index of (i, j) in spectrum.pair_list(N), and writes it with the rows' hits as `P.kmp` (+ `.kmp.json`,
`.kmp.tsv`; query.write_kmp).  hits[row][t] is the diagonal: the windows valid in table t.  A k-mer that occurs twice in the
row counts twice in both.  So every row has what the merger computes for the whole k-mer space -- total_i, total_j,
shared_ij -- restricted to the k-mers of that stretch of the query: where along a chromosome sample A stops looking like B
and starts looking like C is read off the rows' Jaccard distances, or off the trees calculate_distance.py builds from them.

`python -m pykmer_amd.qpairs P.kmp Q --row I` (or `--record NAME [--bin b]`) writes `Q.<min>-<max>.kma` + `.kma.json` for
that row with the merger's writer -- no .kin file, no GPU.
"""
import argparse
import json
import sys
from pathlib import Path
from typing import List

import numpy as np


def load(path) -> dict:
    """`.kmp` and its `.kmp.json` (key `meta`) -> dict(shared, hits, pairs, n_valid, seq_len, kmer_len, min_count, max_count
    [, bin_first, bin_windows[, bin_start, bin_end]], meta)."""
    path = Path(path)
    with np.load(path) as z:
        out = {key: z[key] for key in z.files}
    for key in ("kmer_len", "min_count", "max_count", "bin_windows"):
        if key in out:
            out[key] = int(out[key])
    meta = Path(f"{path}.json")
    if not meta.exists():
        raise ValueError(f"{meta} is missing")
    with meta.open() as fh:
        out["meta"] = json.load(fh)
    return out


def row_matrix(hits_row: np.ndarray, shared_row: np.ndarray) -> np.ndarray:
    """(N, N, 3) uint64, laid out as the merger lays out the `matrix` of a `.kma` (pk_gram_expand): [i][j] = (total_i, total_j,
    shared_ij) for i != j, zeros on the diagonal; total_t = hits_row[t], shared_ij = shared_row[p] of the pair {i, j}."""
    hits_row = np.asarray(hits_row, dtype=np.uint64).reshape(-1)
    shared_row = np.asarray(shared_row, dtype=np.uint64).reshape(-1)
    N = hits_row.size
    if shared_row.size != N * (N - 1) // 2:
        raise ValueError(f"{N} tables have {N * (N - 1) // 2} pairs, got {shared_row.size}")
    upper = np.zeros((N, N), dtype=np.uint64)
    upper[np.triu_indices(N, 1)] = shared_row                # row-major over i < j: the order of spectrum.pair_list
    matrix = np.zeros((N, N, 3), dtype=np.uint64)
    matrix[:, :, 0] = hits_row[:, None]
    matrix[:, :, 1] = hits_row[None, :]
    matrix[:, :, 2] = upper + upper.T
    matrix[np.arange(N), np.arange(N)] = 0
    return matrix


def jaccard(hits: np.ndarray, shared: np.ndarray) -> np.ndarray:
    """(rows, P) float64: the Jaccard distance of every pair in every row, 1 - s / (h_i + h_j - s); 1.0 where neither table
    has a window of the row (the denominator is 0)."""
    hits = np.asarray(hits, dtype=np.uint64)
    shared = np.asarray(shared, dtype=np.uint64)
    assert hits.ndim == 2 and shared.ndim == 2 and hits.shape[0] == shared.shape[0]
    N = hits.shape[1]
    i, j = np.triu_indices(N, 1)
    assert shared.shape[1] == i.size, f"{N} tables have {i.size} pairs, got {shared.shape[1]}"
    union = hits[:, i] + hits[:, j] - shared                 # exact: s <= min(h_i, h_j)
    out = np.ones(shared.shape, dtype=np.float64)
    np.divide(shared.astype(np.float64), union.astype(np.float64), out=out, where=union > 0)
    out[union > 0] = 1.0 - out[union > 0]
    return out


def find_row(kmp: dict, record: str, bin_index: int = None) -> int:
    """The row of the record named `record` (its first, if several carry the name); binned: of its bin `bin_index` [0]."""
    names = list(kmp["meta"]["records"])
    if record not in names:
        raise ValueError(f"no record named {record!r}")
    r = names.index(record)
    if "bin_first" not in kmp:
        if bin_index is not None:
            raise ValueError("--bin chooses a bin of a binned .kmp; this one has one row per record")
        return r
    first, end = int(kmp["bin_first"][r]), int(kmp["bin_first"][r + 1])
    b = 0 if bin_index is None else int(bin_index)
    if not 0 <= b < end - first:
        raise ValueError(f"record {record!r} has {end - first} bins, asked for bin {b}")
    return first + b


def derive(kmp_path, project_name: str, row: int = None, record: str = None, bin_index: int = None) -> np.ndarray:
    """Writes `<project>.<min>-<max>.kma` + `.kma.json` for one row of a `.kmp` through merger.write_kma and returns the
    matrix.  Nothing is overwritten."""
    from .merger import write_kma
    if not Path(kmp_path).exists():
        raise ValueError(f"pairs file does not exist: {kmp_path}")
    if (row is None) == (record is None):
        raise ValueError("choose the row by --row I or by --record NAME")
    kmp = load(kmp_path)
    if row is None:
        row = find_row(kmp, record, bin_index)
    elif bin_index is not None:
        raise ValueError("--bin goes with --record")
    rows = kmp["shared"].shape[0]
    if not 0 <= int(row) < rows:
        raise ValueError(f"the file has {rows} rows, asked for row {row}")
    mn, mx = kmp["min_count"], kmp["max_count"]
    outfile = Path(f"{project_name}.{mn:03d}-{mx:03d}.kma")
    for f in (outfile, Path(f"{outfile}.json")):
        if f.exists():
            raise ValueError(f"project output file ({f}) already exists. not overwriting.")
    matrix = row_matrix(kmp["hits"][int(row)], kmp["shared"][int(row)])
    write_kma(project_name, mn, mx, kmp["meta"]["data"], matrix)
    return matrix


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Write one row of a query's shared k-mers (.kmp) as a .kma matrix: no tables, no GPU.")
    parser.add_argument("Pairs", metavar="S", type=Path, help="<project>.kmp written by query.py --pairs")
    parser.add_argument("Project_Name", metavar="P", type=str, help="Project name (prefix of the output files)")
    parser.add_argument("--row", type=int, default=None, metavar="I", help="The row: a record, or for a binned .kmp a bin, by its index")
    parser.add_argument("--record", type=str, default=None, metavar="NAME", help="The row by the name of its record")
    parser.add_argument("--bin", type=int, default=None, metavar="b", dest="bin_index", help="With --record, binned .kmp: the bin of the record [0]")
    return parser


def main(argv: List[str] = None) -> None:
    args = build_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    try:
        matrix = derive(args.Pairs, args.Project_Name, args.row, args.record, args.bin_index)
    except ValueError as exc:
        print(f"error: {exc}", file=sys.stderr)
        sys.exit(1)
    print(f"{matrix.shape[0]} tables, {matrix.shape[0] * (matrix.shape[0] - 1) // 2} pairs")


if __name__ == "__main__":
    main()
