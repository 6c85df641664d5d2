"""kWIP's entropy-weighted inner-product kernel and distance over the merger's tables.

kWIP (Murray et al. 2017) weights each k-mer by how informative it is across the sample set: the Shannon entropy of its
occupancy o(x) = #{i : c_i(x) >= 1} among the N samples, w(o) = H(o/N), so a k-mer held by every sample (or none) weighs 0.
Because the weight depends on x only through o(x), one GPU pass (k_occgram, pk_occgram_device_accumulate) reduces the
tables to exact integers, and every weighting is host float64 over them:

  occ_hist[o]      #{x : o(x) = o}, o = 0..N
  lin[o-1][i]      sum_{x : o(x) = o} c_i(x)
  gram[o-1][p]     sum_{x : o(x) = o} c_i(x) c_j(x), p = (i, j), i <= j (pair_list order)

  S_i = sum_o lin[o-1][i]                                  (table i's value sum)
  K(i, j) = sum_{o=1..N} w(o) G[o][i][j] / (S_i S_j)       (summed in increasing o; 0 where S_i S_j = 0)
  D(i, j) = sqrt(max(0, 2 - 2 K(i, j) / sqrt(K(i, i) K(j, j)))),  D(i, i) = 0;  rows with K(i, i) = 0 are nan

`merger.py P a.kin b.kin ... --kwip` writes

  <P>.kmo        np.savez_compressed: occ_hist (N+1,), lin (N, N), gram (N, T) u64, pairs (T, 2) int32, kmer_len, data_size
  <P>.kmo.json   project_name, kmer_len, data_size, data (the `data` list merge() writes into a .kma.json)
  <P>.kern       the kernel K, kWIP's TSV layout: a tab and the names, then one line per sample: its name and %.17g values
  <P>.dist       the distance D, same layout

and `python -m pykmer_amd.kwip P.kmo [--kernel F] [--distance F] [--unweighted]` writes either matrix again from the .kmo
alone (no tables, no GPU); --unweighted sets w = 1.
"""
import argparse
import json
import sys
from pathlib import Path
from typing import List, Tuple

import numpy as np

from . import _lib
from .output import atomic_write, write_json


def pair_list(N: int) -> np.ndarray:
    """(T, 2) int32: the pairs i <= j in row-major upper-triangle order, diagonal included (the order of gram's columns)."""
    return np.array([(i, j) for i in range(N) for j in range(i, N)], dtype=np.int32).reshape(-1, 2)


def split_accumulator(acc: np.ndarray, N: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Flat accumulator (pk_occgram_device_accumulate's layout) -> occ_hist (N+1,), lin (N, N), gram (N, T): views."""
    acc = np.asarray(acc).view(np.uint64)
    assert acc.size == _lib.occgram_words(N), (acc.size, N)
    return acc[: N + 1], acc[N + 1: N + 1 + N * N].reshape(N, N), acc[N + 1 + N * N:].reshape(N, -1)


def weights(N: int, unweighted: bool = False) -> np.ndarray:
    """w[o] for o = 0..N: the binary entropy H(o / N) in bits (w[0] = w[N] = 0), or all ones."""
    if unweighted:
        return np.ones(N + 1, dtype=np.float64)
    w = np.zeros(N + 1, dtype=np.float64)
    for o in range(1, N):
        p = min(o, N - o) / N                                  # H(p) = H(1 - p), and w(o) = w(N - o) exactly
        w[o] = -p * np.log2(p) - (1.0 - p) * np.log2(1.0 - p)
    return w


def kernel(lin: np.ndarray, gram: np.ndarray, w: np.ndarray) -> np.ndarray:
    """The N x N float64 kernel K from the class-stratified tallies and per-class weights w[0..N]."""
    N = lin.shape[1]
    acc = np.zeros(gram.shape[1], dtype=np.float64)
    for o in range(1, N + 1):                                  # increasing o: the summation order is part of the contract
        acc += w[o] * gram[o - 1].astype(np.float64)
    s = lin.astype(np.float64).sum(axis=0)
    pairs = pair_list(N)
    k = np.zeros((N, N), dtype=np.float64)
    norm = s[pairs[:, 0]] * s[pairs[:, 1]]
    vals = np.divide(acc, norm, out=np.zeros_like(acc), where=norm > 0)
    k[pairs[:, 0], pairs[:, 1]] = vals
    k[pairs[:, 1], pairs[:, 0]] = vals
    return k


def distance(k: np.ndarray, names=None) -> np.ndarray:
    """kWIP's distance from the cosine-normalised kernel; a sample with K(i, i) = 0 gets a nan row and column (and a
    warning on stderr)."""
    N = k.shape[0]
    diag = np.diag(k).copy()
    empty = diag == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = k / np.sqrt(np.outer(diag, diag))
        d = np.sqrt(np.maximum(0.0, 2.0 - 2.0 * cos))
    np.fill_diagonal(d, 0.0)
    for i in np.flatnonzero(empty):
        name = names[i] if names is not None else str(i)
        print(f"warning: sample {name} has a zero kernel norm (no weighted k-mers): its distances are nan", file=sys.stderr)
        d[i, :] = np.nan
        d[:, i] = np.nan
    return d


def matrices(occ: dict, unweighted: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """(K, D) of a loaded .kmo."""
    N = occ["lin"].shape[0]
    k = kernel(occ["lin"], occ["gram"], weights(N, unweighted))
    return k, distance(k, names(occ) if "meta" in occ else None)


def kmo_paths(project_name: str) -> Tuple[Path, Path, Path, Path]:
    return Path(f"{project_name}.kmo"), Path(f"{project_name}.kmo.json"), Path(f"{project_name}.kern"), Path(f"{project_name}.dist")


def names(occ: dict) -> List[str]:
    return [d["header"]["input_file_name"] for d in occ["meta"]["data"]]


def write_matrix(path, m: np.ndarray, ids: List[str]) -> None:
    """kWIP's TSV: header line of a tab and the names, then per sample its name and values (%.17g); through .tmp + rename,
    never over an existing file."""
    path = Path(path)
    assert not path.exists(), f"output file ({path}) already exists. not overwriting."
    with atomic_write(path, "wt") as fh:
        fh.write("\t" + "\t".join(ids) + "\n")
        for name, row in zip(ids, m):
            fh.write(name + "\t" + "\t".join("%.17g" % float(x) for x in row) + "\n")


def save(project_name: str, occ_hist, lin, gram, kmer_len: int, data_size: int, data) -> Tuple[Path, Path]:
    """Writes `<project>.kmo` and `.kmo.json` (each through `.tmp` + rename; neither overwrites an existing file)."""
    kmo, kmo_json = kmo_paths(project_name)[:2]
    for f in (kmo, kmo_json):
        assert not f.exists(), f"kwip output file ({f}) already exists. not overwriting."
    N = lin.shape[0]
    meta = {"project_name": project_name, "kmer_len": int(kmer_len), "data_size": int(data_size), "data": data}
    write_json(kmo_json, meta)
    with atomic_write(kmo, "wb") as fhd:
        np.savez_compressed(fhd, occ_hist=np.ascontiguousarray(occ_hist, dtype=np.uint64), lin=np.ascontiguousarray(lin, dtype=np.uint64),
                            gram=np.ascontiguousarray(gram, dtype=np.uint64), pairs=pair_list(N), kmer_len=np.int64(kmer_len),
                            data_size=np.int64(data_size))
    return kmo, kmo_json


def check(occ: dict) -> None:
    """The invariants every .kmo satisfies (AssertionError otherwise)."""
    occ_hist, lin, gram = occ["occ_hist"], occ["lin"], occ["gram"]
    N = lin.shape[0]
    assert occ_hist.shape == (N + 1,) and gram.shape == (N, N * (N + 1) // 2), "array shapes disagree with N"
    assert int(occ_hist.sum(dtype=np.uint64)) == occ["data_size"], "occupancy histogram does not sum to data_size"
    diag = np.array([p for p, (i, j) in enumerate(pair_list(N)) if i == j])
    off = np.setdiff1d(np.arange(gram.shape[1]), diag)
    assert not gram[0, off].any(), "class 1 has a cross product (a k-mer held by one sample only)"
    assert np.array_equal(lin == 0, gram[:, diag] == 0), "lin and the gram diagonal disagree on which (class, sample) is empty"


def load(path) -> dict:
    """`.kmo` (and its `.kmo.json`, when present: key `meta`) -> dict(occ_hist, lin, gram, pairs, kmer_len, data_size[, meta]),
    its invariants checked."""
    path = Path(path)
    with np.load(path) as z:
        out = {k: z[k] for k in ("occ_hist", "lin", "gram", "pairs")}
        out["kmer_len"], out["data_size"] = int(z["kmer_len"]), int(z["data_size"])
    check(out)
    meta = Path(f"{path}.json")
    if meta.exists():
        with meta.open() as fh:
            out["meta"] = json.load(fh)
    return out


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="kWIP kernel / distance matrices from a .kmo: no tables, no GPU.")
    parser.add_argument("Occ", metavar="O", type=Path, help="<project>.kmo written by merger.py --kwip")
    parser.add_argument("--kernel", type=Path, default=None, help="write the kernel matrix here")
    parser.add_argument("--distance", type=Path, default=None, help="write the distance matrix here")
    parser.add_argument("--unweighted", action="store_true", help="weight every occupancy class 1 instead of by its entropy")
    return parser


def main(argv: List[str] = None) -> None:
    parser = build_parser()
    args = parser.parse_args(sys.argv[1:] if argv is None else argv)
    if args.kernel is None and args.distance is None:
        parser.error("nothing to write: give --kernel and/or --distance")
    for f in (args.kernel, args.distance):
        if f is not None and f.exists():
            parser.error(f"output file ({f}) already exists. not overwriting.")
    occ = load(args.Occ)
    if "meta" not in occ:
        parser.error(f"{args.Occ}.json is missing")
    k, d = matrices(occ, args.unweighted)
    if args.kernel is not None:
        write_matrix(args.kernel, k, names(occ))
    if args.distance is not None:
        write_matrix(args.distance, d, names(occ))


if __name__ == "__main__":
    main()
