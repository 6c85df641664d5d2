"""Per-record count spectra of a query: every --min-count / --max-count window, the median and any quantile from ONE lookup.

`query.py P Q K... --spectrum` tallies, per row (a record of the query, or a bin of `--bin W`) and table t, how many of the
row's valid windows a_1 .. a_m have each table count,
    spectrum[row][t][c] = #{ j : T_t[a_j] == c }        c = 0 .. 255 (0: the k-mer is absent), uint64, exact
and writes it as `P.kmh` (+ `.kmh.json`, `.kmh.tsv`; query.write_kmh).  The count window of the run plays no part in it, so
    spectrum[row][t].sum() == m
    hits(A, B)  = sum of spectrum[c]      over c = A .. B
    depth(A, B) = sum of c * spectrum[c]  over c = A .. B
are what a run with the window [A, B] gives, and the lower median of the m counts, zeros included -- the robust k-mer
coverage of a contig or a bin, where depth / hits is a mean that a few repeat k-mers dominate -- is the smallest c with
sum of spectrum[v] over v <= c  >=  (m - 1) // 2 + 1  (0 when m = 0).

`python -m pykmer_amd.qspectrum P.kmh Q [--min-count A --max-count B]` derives `Q.kmq` (+ `.kmq.json`, `.kmq.tsv`; for a
binned `.kmh` also the `Q.kmb` files, without coordinates) from it -- no .kin file, no GPU -- equal to what
`query.py Q ... --min-count A --max-count B` writes.
"""
import argparse
import json
import sys
from pathlib import Path
from typing import List, Tuple

import numpy as np


def window_from_spectrum(spectrum: np.ndarray, min_count: int, max_count: int) -> Tuple[np.ndarray, np.ndarray]:
    """(hits, depth), uint64, of the count window [min_count, max_count] from spectra whose last axis is the 256 counts."""
    spectrum = np.asarray(spectrum, dtype=np.uint64)
    assert spectrum.shape[-1] == 256, "the last axis of a spectrum holds the counts 0 .. 255"
    if not 1 <= min_count <= max_count <= 255:
        raise ValueError(f"the count window must satisfy 1 <= min <= max <= 255, got {min_count}-{max_count}")
    part = spectrum[..., int(min_count):int(max_count) + 1]
    counts = np.arange(int(min_count), int(max_count) + 1, dtype=np.uint64)
    return part.sum(axis=-1, dtype=np.uint64), (part * counts).sum(axis=-1, dtype=np.uint64)


def median_from_spectrum(spectrum: np.ndarray) -> np.ndarray:
    """uint8, one per spectrum: the lower median of its m = spectrum.sum() counts, zeros included -- the smallest c with
    sum(spectrum[.. c]) >= (m - 1) // 2 + 1; 0 for m = 0."""
    spectrum = np.asarray(spectrum, dtype=np.uint64)
    assert spectrum.shape[-1] == 256, "the last axis of a spectrum holds the counts 0 .. 255"
    cum = np.cumsum(spectrum, axis=-1, dtype=np.uint64)
    m = cum[..., -1:]
    need = np.where(m > 0, (m - np.minimum(m, 1)) // np.uint64(2) + np.uint64(1), np.uint64(0))
    return (cum < need).sum(axis=-1).astype(np.uint8)        # the counts whose cumulative tally falls short lie below it


def load(path) -> dict:
    """`.kmh` and its `.kmh.json` (key `meta`) -> dict(spectrum, median, n_valid, seq_len, kmer_len[, bin_first, bin_windows], meta)."""
    path = Path(path)
    with np.load(path) as z:
        out = {key: z[key] for key in z.files}
    out["kmer_len"] = int(out["kmer_len"])
    if "bin_windows" in out:
        out["bin_windows"] = int(out["bin_windows"])
    meta = Path(f"{path}.json")
    if not meta.exists():
        raise ValueError(f"{meta} is missing")
    with meta.open() as fh:
        out["meta"] = json.load(fh)
    return out


def derive(kmh_path, project_name: str, min_count: int = 1, max_count: int = 255) -> dict:
    """Writes `<project>.kmq` + `.kmq.json` + `.kmq.tsv` (and the three `.kmb` files for a binned `.kmh`) for the window
    through the writers of a direct run; returns the result they were given.  Nothing is overwritten."""
    from .query import kmb_paths, kmq_paths, record_sums, write_kmb, write_kmq
    if not 1 <= min_count <= max_count <= 255:
        raise ValueError(f"the count window must satisfy 1 <= min <= max <= 255, got {min_count}-{max_count}")
    if not Path(kmh_path).exists():
        raise ValueError(f"spectrum file does not exist: {kmh_path}")
    spec = load(kmh_path)
    binned = "bin_first" in spec
    for f in kmq_paths(project_name) + (kmb_paths(project_name) if binned else ()):
        if f.exists():
            raise ValueError(f"project output file ({f}) already exists. not overwriting.")
    meta = spec["meta"]
    hits, depth = window_from_spectrum(spec["spectrum"], min_count, max_count)
    result = {"names": list(meta["records"]), "n_valid": spec["n_valid"], "seq_len": spec["seq_len"], "kmer_len": spec["kmer_len"],
              "min_count": int(min_count), "max_count": int(max_count)}
    if meta.get("min_qual"):
        result.update(min_qual=meta["min_qual"], qual_offset=meta["qual_offset"])
    if binned:
        result.update(bin_hits=hits, bin_depth=depth, bin_first=spec["bin_first"], bin_windows=spec["bin_windows"],
                      hits=record_sums(hits, spec["bin_first"]), depth=record_sums(depth, spec["bin_first"]))
    else:
        result.update(hits=hits, depth=depth)
    columns = [str(d["header"]["project_name"]) for d in meta["data"]]
    write_kmq(project_name, result, meta["query_file"], meta["data"], columns)
    if binned:
        write_kmb(project_name, result, meta["query_file"], meta["data"], columns)
    return result


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Derive .kmq (and .kmb) files from the count spectra of a query (.kmh): no tables, no GPU.")
    parser.add_argument("Spectrum", metavar="S", type=Path, help="<project>.kmh written by query.py --spectrum")
    parser.add_argument("Project_Name", metavar="P", type=str, help="Project name (prefix of the output files)")
    parser.add_argument("--min-count", type=int, default=1, help="Minimum Kmer Count [1]")
    parser.add_argument("--max-count", type=int, default=255, help="Maximum Kmer Count [255]")
    return parser


def main(argv: List[str] = None) -> None:
    args = build_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    try:
        result = derive(args.Spectrum, args.Project_Name, args.min_count, args.max_count)
    except ValueError as exc:
        print(f"error: {exc}", file=sys.stderr)
        sys.exit(1)
    print(f"{len(result['names'])} records, {result['hits'].shape[1]} tables, count window {args.min_count}-{args.max_count}")


if __name__ == "__main__":
    main()
