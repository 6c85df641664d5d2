"""Presence patterns: how many k-mers each subset of the tables holds, from ONE pass over the tables.

For tables t = 0 .. N-1 (matrix order; 1 <= N <= 16) and a count window 1 <= min <= max <= 255

  m(x) = sum_t [min <= T_t[x] <= max] << t          for every address x in [0, 4^k)
  patterns[p] = #{x : m(x) = p}                      p = 0 .. 2^N - 1, uint64, exact

so patterns.sum() == data_size and patterns[0] counts the addresses no table holds in the window.  This is the data behind
a Venn or UpSet plot: the k-mers private to a table are patterns[1 << i], the core is patterns[2^N - 1], and every pair
tally, occupancy class, intersection, union and difference of any subset is a sum over the bins (matrix_from_patterns,
occupancy_from_patterns, count_where).  `merger.py P a.kin b.kin ... --patterns` makes the pass (k_patterns,
pk_patterns_device_accumulate) and writes, per window,

  <P>.<min>-<max>.kmv        np.savez_compressed: patterns (2^N,) u64, n_tables, kmer_len, data_size, min_count, max_count
  <P>.<min>-<max>.kmv.json   the keys of the .kma.json, kmer_len, data_size, n_tables, n_patterns (non-zero bins other than
                             bin 0), pan (data_size - patterns[0]), core, private (N values)
  <P>.<min>-<max>.kmv.tsv    UpSet input: one 0/1 column per table (its project_name), n_tables and count; one line per
                             non-zero bin other than bin 0, by count descending, then pattern ascending

and `python -m pykmer_amd.patterns P.kmv [--all-of a,b] [--none-of c] [--any-of d,e] [--kma Q]` answers from the .kmv alone
(no .kin file, no GPU): the count of a condition, tables given by index or project_name, and / or `Q.<min>-<max>.kma` +
`.kma.json` for calculate_distance.py.
"""
import argparse
import json
import sys
from pathlib import Path
from typing import List, Sequence, Tuple

import numpy as np

from .output import atomic_write, write_json

MAX_TABLES = 16                                              # 2^N bins as a dense array


def check_tables(N: int) -> None:
    if not 1 <= N <= MAX_TABLES:
        raise ValueError(f"presence patterns take 1 to {MAX_TABLES} tables, got {N}: the 2^N bins are kept as a dense array")


def _bins(patterns, N: int) -> np.ndarray:
    check_tables(N)
    p = np.ascontiguousarray(patterns, dtype=np.uint64)
    assert p.shape == (1 << N,), f"{N} tables have {1 << N} patterns, got an array of shape {p.shape}"
    return p


def _bits(N: int) -> np.ndarray:
    """(2^N, N) uint64: [p][t] = bit t of p."""
    return (np.arange(1 << N, dtype=np.uint64)[:, None] >> np.arange(N, dtype=np.uint64)[None, :]) & np.uint64(1)


def matrix_from_patterns(patterns, N: int) -> np.ndarray:
    """The N x N u64 that merger.pair_matrix returns for the window: [i][i] = the addresses table i holds, [i][j] (i < j) =
    those both hold, below the diagonal 0 (expand it with _lib.gram_expand)."""
    p = _bins(patterns, N)
    b = _bits(N)
    return np.triu((b.T * p[None, :]) @ b)                     # integer matmul in u64: exact


def occupancy_from_patterns(patterns, N: int) -> np.ndarray:
    """(N + 1,) u64: the addresses held by exactly o tables, o = 0 .. N."""
    p = _bins(patterns, N)
    held = _bits(N).sum(axis=1)
    return np.array([p[held == o].sum(dtype=np.uint64) for o in range(N + 1)], dtype=np.uint64)


def _mask(tables, N: int, what: str) -> int:
    m = 0
    for t in tables:
        t = int(t)
        if not 0 <= t < N:
            raise ValueError(f"{what}: table {t} is not one of the {N} tables")
        m |= 1 << t
    return m


def count_where(patterns, N: int, all_of: Sequence[int] = (), none_of: Sequence[int] = (), any_of: Sequence[int] = ()) -> int:
    """The addresses whose pattern has every bit of `all_of`, no bit of `none_of` and, if given, at least one of `any_of`."""
    p = _bins(patterns, N)
    need, ban, some = _mask(all_of, N, "all_of"), _mask(none_of, N, "none_of"), _mask(any_of, N, "any_of")
    idx = np.arange(1 << N, dtype=np.int64)
    sel = ((idx & need) == need) & ((idx & ban) == 0)
    if len(tuple(any_of)):
        sel &= (idx & some) != 0
    return int(p[sel].sum(dtype=np.uint64))


def pattern_paths(project_name: str, min_count: int, max_count: int) -> Tuple[Path, Path, Path]:
    kmv = f"{project_name}.{min_count:03d}-{max_count:03d}.kmv"
    return Path(kmv), Path(kmv + ".json"), Path(kmv + ".tsv")


def table_names(data) -> List[str]:
    return [str(d["header"]["project_name"]) for d in data]


def save(project_name: str, min_count: int, max_count: int, patterns, kmer_len: int, data_size: int, data) -> Tuple[Path, Path, Path]:
    """Writes `<project>.<min>-<max>.kmv`, `.kmv.json` and `.kmv.tsv` (each through `.tmp` + rename; none overwrites an
    existing file).  `data`: the list merge() writes into a .kma.json, headers already lean."""
    N = len(data)
    p = _bins(patterns, N)
    assert int(p.sum(dtype=np.uint64)) == int(data_size), "the patterns do not sum to data_size"
    kmv, kmv_json, kmv_tsv = pattern_paths(project_name, min_count, max_count)
    for f in (kmv, kmv_json, kmv_tsv):
        assert not f.exists(), f"pattern output file ({f}) already exists. not overwriting."
    rest = np.flatnonzero(p[1:]) + 1
    meta = {"project_name": project_name, "min_count": int(min_count), "max_count": int(max_count), "data": data,
            "kmer_len": int(kmer_len), "data_size": int(data_size), "n_tables": N, "n_patterns": int(rest.size),
            "pan": int(data_size) - int(p[0]), "core": int(p[-1]), "private": [int(p[1 << i]) for i in range(N)]}
    write_json(kmv_json, meta)
    order = rest[np.lexsort((rest, _descending(p[rest])))]     # by count from the largest down, then by pattern
    with atomic_write(kmv_tsv, "wt") as fh:
        fh.write("\t".join(table_names(data) + ["n_tables", "count"]) + "\n")
        for q in order:
            q = int(q)
            fh.write("\t".join([str((q >> t) & 1) for t in range(N)] + [str(bin(q).count("1")), str(int(p[q]))]) + "\n")
    with atomic_write(kmv, "wb") as fhd:
        np.savez_compressed(fhd, patterns=p, n_tables=np.int64(N), kmer_len=np.int64(kmer_len), data_size=np.int64(data_size),
                            min_count=np.int64(min_count), max_count=np.int64(max_count))
    return kmv, kmv_json, kmv_tsv


def _descending(counts: np.ndarray) -> np.ndarray:
    """A sort key that orders u64 counts from the largest down (exact: no float, no negation of unsigned values)."""
    return np.uint64(0xFFFFFFFFFFFFFFFF) - counts


def load(path) -> dict:
    """`.kmv` (and its `.kmv.json`, when present: key `meta`) -> dict(patterns, n_tables, kmer_len, data_size, min_count,
    max_count[, meta]); the patterns sum to data_size (AssertionError otherwise)."""
    path = Path(path)
    with np.load(path) as z:
        out = {"patterns": z["patterns"].astype(np.uint64)}
        for key in ("n_tables", "kmer_len", "data_size", "min_count", "max_count"):
            out[key] = int(z[key])
    assert out["patterns"].shape == (1 << out["n_tables"],), "array shape disagrees with n_tables"
    assert int(out["patterns"].sum(dtype=np.uint64)) == out["data_size"], "the patterns do not sum to data_size"
    meta = Path(f"{path}.json")
    if meta.exists():
        with meta.open() as fh:
            out["meta"] = json.load(fh)
    return out


def write_window_kma(project_name: str, kmv: dict):
    """`<project>.<min>-<max>.kma` + `.kma.json` of a loaded .kmv (with its meta); returns the (N, N, 3) matrix."""
    from . import _lib
    from .merger import print_matrix, write_kma
    mn, mx = kmv["min_count"], kmv["max_count"]
    outfile = Path(f"{project_name}.{mn:03d}-{mx:03d}.kma")
    assert not Path(project_name).exists(), f"project name ({project_name}) is a file. maybe forgot to pass project name as first argument?"
    for f in (outfile, Path(f"{outfile}.json")):
        assert not f.exists(), f"project output file ({f}) already exists. not overwriting."
    matrix = _lib.gram_expand(matrix_from_patterns(kmv["patterns"], kmv["n_tables"]))
    print_matrix(matrix)
    write_kma(project_name, mn, mx, kmv["meta"]["data"], matrix)
    return matrix


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Counts and .kma matrices from presence patterns (.kmv): no tables, no GPU.")
    parser.add_argument("Patterns", metavar="V", type=Path, help="<project>.<min>-<max>.kmv written by merger.py --patterns")
    parser.add_argument("--all-of", type=str, default="", help="tables that must all hold the k-mer: indices or project names, comma-separated")
    parser.add_argument("--none-of", type=str, default="", help="tables that must not hold it")
    parser.add_argument("--any-of", type=str, default="", help="tables of which at least one must hold it")
    parser.add_argument("--kma", type=str, default=None, metavar="Q", help="write Q.<min>-<max>.kma + .kma.json for calculate_distance.py")
    return parser


def _resolve(text: str, names: List[str], N: int) -> List[int]:
    out = []
    for item in (s.strip() for s in text.split(",")):
        if item == "":
            continue
        if item in names:
            out.append(names.index(item))
        elif item.isdigit() and int(item) < N:
            out.append(int(item))
        else:
            raise ValueError(f"unknown table {item!r}: give an index below {N} or one of {', '.join(names) if names else 'the indices'}")
    return out


def main(argv: List[str] = None) -> None:
    parser = build_parser()
    args = parser.parse_args(sys.argv[1:] if argv is None else argv)
    counting = bool(args.all_of or args.none_of or args.any_of)
    if not counting and args.kma is None:
        parser.error("nothing to do: give --all-of / --none-of / --any-of and/or --kma")
    try:
        kmv = load(args.Patterns)
        N = kmv["n_tables"]
        names = table_names(kmv["meta"]["data"]) if "meta" in kmv else []
        if counting:
            sets = [_resolve(t, names, N) for t in (args.all_of, args.none_of, args.any_of)]
            print(count_where(kmv["patterns"], N, *sets))
        if args.kma is not None:
            if "meta" not in kmv:
                raise ValueError(f"{args.Patterns}.json is missing")
            write_window_kma(args.kma, kmv)
    except (ValueError, AssertionError, OSError) as e:
        print(f"error: {e}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
