"""Joint count spectra: every --min-count / --max-count window of a merge from ONE pass over the tables.

The reference tallies a pair under one validity window (Header.calculate_distance, tools.py:473-482) and runs the whole
merge again for every other window (README.md:57-61).  Per pair (i < j) the joint count spectrum
J_ij[a][b] = #{x : c_i(x) = a, c_j(x) = b} (256 x 256 u64) holds every window: shared_ij(lo, hi) is the box sum of J_ij
over [lo, hi]^2 and total_i(lo, hi) the sum of table i's value histogram over [lo, hi].  `merger.py ... --spectrum` makes
that pass (k_spectrum) and writes

  <project>.kms        np.savez_compressed: hist (N, 256) u64, joint (P, 256, 256) u64 (P = N(N-1)/2, pairs i < j
                       row-major), pairs (P, 2) int32, kmer_len, data_size
  <project>.kms.json   project_name, kmer_len, data_size, data (the `data` list merge() writes into a .kma.json)

and `python -m pykmer_amd.spectrum P.kms Q [--min-count A --max-count B | --sweep 1-255,1-50,...]` derives
`Q.<min>-<max>.kma` + `.kma.json` from it -- no .kin file, no GPU.
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
    """(P, 2) int32: the pairs i < j in row-major upper-triangle order (the order of the joint spectra)."""
    return np.array([(i, j) for i in range(N) for j in range(i + 1, N)], dtype=np.int32).reshape(-1, 2)


def split_accumulator(acc: np.ndarray, N: int) -> Tuple[np.ndarray, np.ndarray]:
    """Flat accumulator (pk_spectrum_device_accumulate's layout) -> hist (N, 256), core (P, 255, 255): views, no copy."""
    acc = np.asarray(acc).view(np.uint64)
    assert acc.size == _lib.spectrum_words(N), (acc.size, N)
    return acc[: N * 256].reshape(N, 256), acc[N * 256:].reshape(-1, 255, 255)


def expand(hist: np.ndarray, core: np.ndarray, n: int) -> np.ndarray:
    """The full joint[P][256][256] from the histograms and the joint bins of counts >= 1: row / column 0 come from the
    marginals (joint[p][a][0] = hist[i][a] - sum_{b>=1} core[p][a][b]) and [0][0] closes the sum to n."""
    N = hist.shape[0]
    hist = hist.astype(np.int64)
    joint = np.zeros((len(core), 256, 256), dtype=np.uint64)
    for p, (i, j) in enumerate(pair_list(N)):
        c = core[p].astype(np.int64)
        rows = hist[i, 1:] - c.sum(axis=1)
        cols = hist[j, 1:] - c.sum(axis=0)
        corner = int(n) - int(c.sum()) - int(rows.sum()) - int(cols.sum())
        assert (rows >= 0).all() and (cols >= 0).all() and corner >= 0, f"pair {i},{j}: spectrum inconsistent with the histograms"
        joint[p, 1:, 1:] = core[p]
        joint[p, 1:, 0] = rows
        joint[p, 0, 1:] = cols
        joint[p, 0, 0] = corner
    return joint


def expand_accumulator(acc: np.ndarray, N: int, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """Flat accumulator -> (hist (N, 256) u64, joint (P, 256, 256) u64)."""
    hist, core = split_accumulator(acc, N)
    return hist.copy(), expand(hist, core, n)


def window_pairs(hist: np.ndarray, joint: np.ndarray, windows) -> List[np.ndarray]:
    """One N x N u64 per (min_count, max_count) window, laid out as merger.pair_matrix returns it: [i][i] = total_i,
    [i][j] (i < j) = shared_ij, below the diagonal 0 (expand it with _lib.gram_expand).  min > max gives zeros, as
    the reference's mask (tools.py:473-475) does."""
    N = hist.shape[0]
    pairs = pair_list(N)
    out = []
    for mn, mx in windows:
        m = np.zeros((N, N), dtype=np.uint64)
        if mn <= mx:
            lo, hi = int(mn), int(mx) + 1
            m[np.arange(N), np.arange(N)] = hist[:, lo:hi].sum(axis=1, dtype=np.uint64)
            if len(pairs):
                m[pairs[:, 0], pairs[:, 1]] = joint[:, lo:hi, lo:hi].sum(axis=(1, 2), dtype=np.uint64)
        out.append(m)
    return out


def spectrum_paths(project_name: str) -> Tuple[Path, Path]:
    return Path(f"{project_name}.kms"), Path(f"{project_name}.kms.json")


def save(project_name: str, hist: np.ndarray, joint: np.ndarray, kmer_len: int, data_size: int, data) -> Tuple[Path, Path]:
    """Writes `<project>.kms` and `.kms.json` (each through `.tmp` + rename; neither overwrites an existing file)."""
    kms, kms_json = spectrum_paths(project_name)
    for f in (kms, kms_json):
        assert not f.exists(), f"spectrum output file ({f}) already exists. not overwriting."
    N = hist.shape[0]
    meta = {"project_name": project_name, "kmer_len": int(kmer_len), "data_size": int(data_size), "data": data}
    write_json(kms_json, meta)
    with atomic_write(kms, "wb") as fhd:
        np.savez_compressed(fhd, hist=np.ascontiguousarray(hist, dtype=np.uint64), joint=np.ascontiguousarray(joint, dtype=np.uint64),
                            pairs=pair_list(N), kmer_len=np.int64(kmer_len), data_size=np.int64(data_size))
    return kms, kms_json


def load(path) -> dict:
    """`.kms` (and its `.kms.json`, when present: key `meta`) -> dict(hist, joint, pairs, kmer_len, data_size[, meta])."""
    path = Path(path)
    with np.load(path) as z:
        out = {"hist": z["hist"], "joint": z["joint"], "pairs": z["pairs"], "kmer_len": int(z["kmer_len"]), "data_size": int(z["data_size"])}
    meta = Path(f"{path}.json")
    if meta.exists():
        with meta.open() as fh:
            out["meta"] = json.load(fh)
    return out


def build_parser() -> argparse.ArgumentParser:
    from .merger import DEFAULT_MAX_COUNT, DEFAULT_MIN_COUNT
    parser = argparse.ArgumentParser(description="Derive .kma matrices from a joint count spectrum (.kms): no tables, no GPU.")
    parser.add_argument("Spectrum", metavar="S", type=Path, help="<project>.kms written by merger.py --spectrum")
    parser.add_argument("Project_Name", metavar="P", type=str, help="Project name of the .kma files")
    parser.add_argument("--min-count", type=int, default=DEFAULT_MIN_COUNT, nargs="?", help=f"Minimum Kmer Count [{DEFAULT_MIN_COUNT}]")
    parser.add_argument("--max-count", type=int, default=DEFAULT_MAX_COUNT, nargs="?", help=f"Maximum Kmer Count [{DEFAULT_MAX_COUNT}]")
    parser.add_argument("--sweep", type=str, default=None, help="several count windows, e.g. 1-255,1-50 (one .kma each)")
    return parser


def derive(kms_path, project_name: str, windows) -> List[np.ndarray]:
    """Writes `<project>.<min>-<max>.kma` + `.kma.json` for every window from a `.kms`; returns the (N, N, 3) matrices."""
    from .merger import print_matrix, write_kma
    for mn, mx in windows:
        assert mn >= 1
        assert mx <= 255
    outfiles = [Path(f"{project_name}.{mn:03d}-{mx:03d}.kma") for mn, mx in windows]
    assert not Path(project_name).exists(), f"project name ({project_name}) is a file. maybe forgot to pass project name as first argument?"
    for outfile in outfiles:
        assert not outfile.exists(), f"project output file ({outfile}) already exists. not overwriting."
    spec = load(kms_path)
    assert "meta" in spec, f"{kms_path}.json is missing"
    matrices = []
    for (mn, mx), pair in zip(windows, window_pairs(spec["hist"], spec["joint"], windows)):
        matrix = _lib.gram_expand(pair)
        matrices.append(matrix)
        print_matrix(matrix)
        write_kma(project_name, mn, mx, spec["meta"]["data"], matrix)
    return matrices


def main(argv: List[str] = None) -> None:
    from .merger import parse_sweep
    args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    windows = parse_sweep(args.sweep) if args.sweep else [(args.min_count, args.max_count)]
    derive(args.Spectrum, args.Project_Name, windows)


if __name__ == "__main__":
    main()
