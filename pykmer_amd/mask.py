"""Mask host side: a FASTA file and N `.kin[.bgz]` tables in, the same file out with the bases the tables cover marked.

The query is parsed exactly as query.py parses it.  A valid base is a byte of ACGTacgt that is a sequence character of a
record; the valid bases are numbered in text order over all records.  A valid window matches iff min_count <= T_t[a] <=
max_count in at least one table, and a valid base is covered iff it lies in at least one matching window.  The selected
bases are the covered ones, with `invert` the valid bases that are not covered; the output is the input's own bytes at the
same length with only the selected bytes changed -- byte | 0x20 (soft mask), or N with `hard` -- and is not compressed.

Phase 1 (cover_bits) streams the query against the staged tables with pk_query_set_cover: one bit per valid base, OR-ed on
the host over the table groups that the HBM budget makes.  Phase 2 (apply_mask) streams it a second time through
pk_query_set_mask, which needs no tables: a base at the end of a feed may be covered only by a window that ends in the next
feed, so no feed's text can be finished while the lookups still run.  The reference has no such tool; this is the
`bbduk kmask` step.

With `bed` phase 2 also finds the masked INTERVALS on the device (pk_query_set_intervals): the maximal runs of consecutive
positions of one record that all hold selected bases, 0-based and half-open, in the positions of query.py --coords.  They
are written as `<project>.masked.bed`, one line chrom<TAB>start<TAB>end per interval in stream order, where chrom is the
first whitespace-delimited token of the record's name.
"""
import argparse
import os
import sys
from pathlib import Path
from typing import List, Sequence

import numpy as np

from . import _lib
from .indexer import _Input, _mark, input_format
from .merger import DEFAULT_THREADS
from .output import atomic_write, write_json
from .query import as_headers, plan_groups, refuse_files, stage_tables, stream_groups, validate, verified_tables
from .tables import lean_headers

APPLY_FEED = 64 << 20               # phase 2 feeds at most this much at a time: one piece of the library's, handed back whole


def check_fasta(query_file: str) -> None:
    """FASTQ input is refused: writing FASTQ back is filter.py's side of the family."""
    if input_format(str(query_file)) == "fastq":
        raise ValueError(f"mask.py takes FASTA input: {query_file} is FASTQ by its name (filter.py selects whole reads by the same tables)")


def run_cover(query_file: str, kmer_len: int, ptrs, min_count: int, max_count: int, device: int = 0, first: bool = True) -> dict:
    """Streams the query once against the staged tables `ptrs` with the cover bits on.  `first`: also fetch the record names."""
    src = _Input(query_file, keep=first, quiet=not first)
    n_bytes = 0
    with _lib.QueryIndexer(kmer_len, device=device) as q:
        q.set_tables(ptrs, min_count, max_count)
        q.set_cover(True)
        for piece in src.pieces():
            q.feed(piece)
            n_bytes += len(piece)
        fin = q.finish()
        recs = q.records(fin["n_records"])
        cover, n_bases = q.cover(n_bytes)
        timings = q.timings()
    out = {"seq_len": recs["seq_len"].astype(np.uint64), "n_valid": recs["n_valid_kmers"].astype(np.uint64), "cover": cover.copy(),
           "n_bases": n_bases, "n_bytes": n_bytes, "timings": timings}
    if first:
        out["names"] = [nm.decode("utf-8", "replace") for nm in src.names(recs)]
    return out


def or_cover(result, part):
    """stream_groups' join of cover bits: a later group's bits OR-ed into those of the groups before; the first group's part,
    its bits copied, is the result."""
    if result is None:
        part["cover"] = np.array(part["cover"], dtype=np.uint8)
        return part
    assert part["n_bases"] == result["n_bases"], "query changed between table groups"
    result["cover"] |= np.asarray(part["cover"], dtype=np.uint8)
    return result


def cover_bits(query_file: str, tables: Sequence, min_count: int = 1, max_count: int = 255, device: int = 0, hbm_budget: int = None,
               threads: int = DEFAULT_THREADS, stage=None, run=None) -> dict:
    """The cover bits of `query_file` (FASTA; plain, gzip or BGZF) against `tables`: Headers, merger.ResidentTables or
    `.kin[.bgz]` paths.  Returns dict(names, seq_len (R,), n_valid (R,), n_bases, cover (ceil(n_bases / 8),) uint8 -- bit g at
    byte g // 8, bit g % 8, np.unpackbits(bitorder="little") --, kmer_len, n_groups, lookup_s).
    The tables are staged in groups by the HBM budget as query.query_records stages them; every group's bitmap is OR-ed into
    one.  `stage(tables, device)` and `run(query_file, kmer_len, ptrs, min_count, max_count, device, first)` default to
    query.stage_tables and run_cover (the CPU-only tests substitute both)."""
    check_fasta(query_file)
    tables = as_headers(tables, device)
    kmer_len = validate(tables, min_count, max_count)
    result = stream_groups(query_file, tables, kmer_len, plan_groups(tables, kmer_len, device, hbm_budget), min_count, max_count, run or run_cover,
                           or_cover, device, threads, stage or (lambda group, dev: stage_tables(group, dev, threads)))
    assert result["cover"].shape == ((result["n_bases"] + 7) // 8,)
    return result


def count_bits(cover, n_bases: int) -> int:
    """The set bits among the first n_bases of packed cover bits."""
    return int(np.unpackbits(np.asarray(cover, dtype=np.uint8), bitorder="little")[:n_bases].sum(dtype=np.int64))


def apply_mask(query_file: str, cover, n_bases: int, out_file, hard: bool = False, invert: bool = False, device: int = 0,
               intervals: bool = False) -> dict:
    """Writes `query_file` to `out_file` (through `.tmp` + rename, uncompressed) with the selected valid bases marked: those
    whose bit in `cover` (packed as cover_bits returns it, for n_bases bases; the bits may come from anywhere) is set, with
    `invert` the others; lower case, with `hard` N.  Returns dict(masked (R,) uint64, n_masked, n_records, bytes, mask_s); with
    `intervals` also iv_record, iv_start, iv_end ((M,) uint64, stream order), n_intervals and intervals_s.
    ValueError if `cover` does not hold n_bases bits or the file does not hold n_bases valid bases."""
    check_fasta(query_file)
    bits = np.ascontiguousarray(cover, dtype=np.uint8)
    if bits.ndim != 1 or bits.size != (int(n_bases) + 7) // 8:
        raise ValueError(f"{int(n_bases)} bases take {(int(n_bases) + 7) // 8} bytes of cover bits, got an array of shape {bits.shape}")
    src = _Input(query_file, keep=False, quiet=True)
    block = min(APPLY_FEED, max(1 << 20, int(os.environ.get("PK_FEED_PIECE", APPLY_FEED)))) & ~15
    n_bytes = 0
    with _lib.QueryIndexer(1, device=device) as q, atomic_write(out_file, "wb") as fhd:
        q.set_mask(bits, n_bases, hard=hard, invert=invert)
        if intervals:
            q.set_intervals(True)
        text = np.empty(block, dtype=np.uint8)
        for piece in src.pieces():
            view = memoryview(piece)
            for off in range(0, len(view), block):
                q.feed(view[off:off + block])
                fhd.write(memoryview(q.mask_text(text)))
            n_bytes += len(view)
        fin = q.finish()
        try:
            masked, seen = q.mask_counts(fin["n_records"])
        except _lib.PkError as exc:
            if exc.code != _lib.PK_ERR_STATE:
                raise
            raise ValueError(f"{query_file}: {exc}") from exc
        mask_s = q.timings()["mask_s"]
        found = [a.copy() for a in q.intervals()] + [q.interval_seconds()] if intervals else None
    assert seen == n_bases
    out = {"masked": masked.copy(), "n_masked": int(masked.sum()), "n_records": fin["n_records"], "bytes": n_bytes, "mask_s": mask_s}
    if intervals:
        out.update(iv_record=found[0], iv_start=found[1], iv_end=found[2], n_intervals=int(found[0].size), intervals_s=found[3])
        assert int((found[2] - found[1]).sum()) == out["n_masked"], "intervals and masked bases disagree"
    return out


def kmm_paths(project_name: str):
    return Path(f"{project_name}.masked.fa"), Path(f"{project_name}.kmm"), Path(f"{project_name}.kmm.json")


def bed_path(project_name: str) -> Path:
    return Path(f"{project_name}.masked.bed")


def bed_names(names: Sequence[str]) -> List[str]:
    """The BED chrom of every record: the first whitespace-delimited token of its stripped name.  ValueError, naming the
    record, for an empty name and for a token that two records share: either would make the file ambiguous."""
    chroms, first = [], {}
    for r, name in enumerate(names):
        tokens = name.split()
        if not tokens:
            raise ValueError(f"--bed needs a name for every record: record {r + 1} has an empty header")
        if tokens[0] in first:
            raise ValueError(f"--bed needs distinct record names: records {first[tokens[0]] + 1} and {r + 1} both begin with '{tokens[0]}'")
        first[tokens[0]] = r
        chroms.append(tokens[0])
    return chroms


def write_bed(path, chroms: Sequence[str], iv_record, iv_start, iv_end) -> None:
    """One line chrom<TAB>start<TAB>end per interval, in the order given, UTF-8; through `.tmp` + rename."""
    with atomic_write(path, "wb") as fhd:
        lines = [f"{chroms[int(r)]}\t{int(a)}\t{int(b)}\n" for r, a, b in zip(iv_record, iv_start, iv_end)]
        fhd.write("".join(lines).encode("utf-8"))


def mask_records(query_file: str, tables: Sequence, min_count: int = 1, max_count: int = 255, hard: bool = False, invert: bool = False,
                 project_name: str = None, device: int = 0, hbm_budget: int = None, threads: int = DEFAULT_THREADS, stage=None, run=None,
                 apply=None, bed: bool = False) -> dict:
    """Both phases: cover_bits' result, and with `project_name` `<project>.masked.fa` and masked (R,) uint64, n_masked, bytes,
    mask_s, output.  `apply(query_file, cover, n_bases, out_file, hard=, invert=, device=)` defaults to apply_mask.  `bed`
    (with `project_name`): `apply` is called with intervals=True, and the result also holds chroms (bed_names of the record
    names, checked between the phases), iv_record, iv_start, iv_end, n_intervals and intervals_s."""
    result = cover_bits(query_file, tables, min_count, max_count, device=device, hbm_budget=hbm_budget, threads=threads, stage=stage, run=run)
    result.update(hard=bool(hard), invert=bool(invert))
    if project_name is not None:
        out_file = kmm_paths(project_name)[0]
        more = {}
        if bed:
            result["chroms"] = bed_names([n.strip() for n in result["names"]])
            more["intervals"] = True
        done = (apply or apply_mask)(str(query_file), result["cover"], result["n_bases"], out_file, hard=hard, invert=invert, device=device, **more)
        if done["n_records"] != len(result["n_valid"]):
            raise ValueError(f"{query_file} changed between the passes: {done['n_records']} records now, {len(result['n_valid'])} when it was looked up")
        covered = count_bits(result["cover"], result["n_bases"])
        assert done["n_masked"] == (result["n_bases"] - covered if invert else covered), "masked bases and cover bits disagree"
        _mark(f"{out_file} written")
        result.update(masked=done["masked"], n_masked=done["n_masked"], bytes=done["bytes"], mask_s=done["mask_s"], output=str(out_file))
        if bed:
            result.update({key: done[key] for key in ("iv_record", "iv_start", "iv_end", "n_intervals", "intervals_s")})
    return result


def mask(project_name: str, query_file: str, indexes: List[Path], min_count: int = 1, max_count: int = 255, hard: bool = False,
         invert: bool = False, device: int = 0, threads: int = DEFAULT_THREADS, hbm_budget: int = None, stage=None, run=None, apply=None,
         bed: bool = False) -> dict:
    """The CLI's work: validate, look up, apply, write `<project>.masked.fa`, `<project>.kmm` and `<project>.kmm.json`, with
    `bed` also `<project>.masked.bed`; returns mask_records' result.  Every refusal (ValueError) comes before any file is
    written; no file is overwritten."""
    check_fasta(query_file)
    if len(indexes) < 1:
        raise ValueError("a mask needs at least one table")
    out_file, kmm, meta = kmm_paths(project_name)
    refuse_files((out_file, kmm, meta) + ((bed_path(project_name),) if bed else ()), [query_file])
    data, headers = verified_tables(indexes, min_count, max_count, device)
    result = mask_records(query_file, headers, min_count, max_count, hard=hard, invert=invert, project_name=project_name, device=device,
                          hbm_budget=hbm_budget, threads=threads, stage=stage, run=run, apply=apply, bed=bed)
    lean_headers(data)
    names = [n.strip() for n in result["names"]]
    output = {"project_name": project_name, "kmer_len": int(result["kmer_len"]), "min_count": int(min_count), "max_count": int(max_count),
              "query_file": str(query_file), "records": names, "data": data, "mode": "hard" if hard else "soft", "invert": bool(invert),
              "n_records": len(names), "n_bases": int(result["n_bases"]), "n_masked": int(result["n_masked"]), "bytes": int(result["bytes"]),
              "output": result["output"], "lookup_s": result["lookup_s"], "mask_s": result["mask_s"]}
    arrays = {}
    if bed:
        write_bed(bed_path(project_name), result["chroms"], result["iv_record"], result["iv_start"], result["iv_end"])
        result["bed"] = str(bed_path(project_name))
        output.update(bed=result["bed"], n_intervals=int(result["n_intervals"]), intervals_s=result["intervals_s"])
        arrays = {key: np.ascontiguousarray(result[key], dtype=np.uint64) for key in ("iv_record", "iv_start", "iv_end")}
    write_json(meta, output)
    with atomic_write(kmm, "wb") as fhd:
        np.savez_compressed(fhd, **arrays, masked=np.ascontiguousarray(result["masked"], dtype=np.uint64),
                            n_valid=np.ascontiguousarray(result["n_valid"], dtype=np.uint64),
                            seq_len=np.ascontiguousarray(result["seq_len"], dtype=np.uint64), kmer_len=np.int64(result["kmer_len"]),
                            min_count=np.int64(min_count), max_count=np.int64(max_count), hard=np.bool_(hard), invert=np.bool_(invert),
                            n_bases=np.uint64(result["n_bases"]))
    _mark("files renamed")
    return result


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Mask the bases of a FASTA file that kmer databases cover.")
    parser.add_argument("Project_Name", metavar="P", type=str, help="Project name (prefix of the output files)")
    parser.add_argument("Query", metavar="Q", type=str, help="query.fa[.gz|.bgz]")
    parser.add_argument("Kmer_N", metavar="K", type=Path, nargs="+", help="List of kin files")
    parser.add_argument("--min-count", type=int, default=1, help="Minimum Kmer Count [1]")
    parser.add_argument("--max-count", type=int, default=255, help="Maximum Kmer Count [255]")
    parser.add_argument("--hard", action="store_true", help="Replace the masked bases by N instead of lower-casing them [off]")
    parser.add_argument("--invert", action="store_true", help="Mask the valid bases that no table covers [off]")
    parser.add_argument("--bed", action="store_true", help="Also write the masked intervals as <P>.masked.bed [off]")
    parser.add_argument("--threads", type=int, default=DEFAULT_THREADS, help=f"Host threads reading / inflating the tables [{DEFAULT_THREADS}]")
    parser.add_argument("--min-qual", type=int, default=None, metavar="Q", help="Refused: base qualities belong to FASTQ input, which filter.py takes")
    return parser


def main(argv: List[str] = None) -> None:
    args = build_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    try:
        if args.min_qual is not None:
            raise ValueError("--min-qual needs FASTQ input, which mask.py does not write back: filter.py --min-qual selects whole reads")
        result = mask(args.Project_Name, args.Query, args.Kmer_N, min_count=args.min_count, max_count=args.max_count, hard=args.hard,
                      invert=args.invert, device=int(os.environ.get("PK_DEVICE", "0")), threads=args.threads, bed=args.bed)
    except ValueError as exc:
        print(f"error: {exc}", file=sys.stderr)
        sys.exit(1)
    tail = f", {result['n_intervals']} intervals in {result['bed']}" if args.bed else ""
    print(f"{result['n_masked']} of {result['n_bases']} valid bases masked in {len(result['n_valid'])} records, {result['output']}{tail}")
