"""Filter host side: a FASTA / FASTQ file and N `.kin[.bgz]` tables in, the records that match the tables out.

Phase 1 is the query as it stands (query.query_records: one lookup, the tables staged in groups): per record r and table t
the hits and the valid windows.  The rule, on the host in exact integer arithmetic:
    table t matches record r  iff  hits[r][t] >= H  and  100 * hits[r][t] >= P * n_valid[r]   (never without a valid window)
    record r matches          iff  at least M tables match it
and the matching records are kept, or with `invert` the others (decontamination).  With a mate file record r of both files
is one pair, which matches if either mate does (`any`) or both do (`both`); both files get the same flags.

Phase 2 streams the input a second time through a _lib.Selector (pk_select_*, kmer_select.hip): record r is the bytes from
its '>' or '@' up to the next record's -- [name_off[r] - 1, name_off[r + 1] - 1), the last one to the end of the stream, the
text before the first header dropped -- and the kept records leave the device as the input's own bytes, whatever the format
and the compression of the input.  `--min-qual` changes which reads match, never a byte that is written.
The reference has no such tool (its README stops at the distance matrix); this is the `bbduk` / `kat filter seq` step.
"""
import argparse
import os
import sys
from pathlib import Path
from typing import List, Sequence

import numpy as np

from . import _lib
from .indexer import _Input, _mark, input_format, qual_threshold
from .merger import DEFAULT_THREADS
from .output import atomic_write, write_json
from .query import _qual_keys, as_headers, query_records, refuse_files, verified_tables
from .tables import lean_headers

PAIR_RULES = ("any", "both")


def validate_rule(min_hits, min_percent, min_tables, n_tables: int) -> None:
    """H >= 1, 0 <= P <= 100, 1 <= M <= N, all integers (a bool or a float is none); ValueError otherwise."""
    for name, v in (("--min-hits", min_hits), ("--min-percent", min_percent), ("--min-tables", min_tables)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if min_hits < 1:
        raise ValueError(f"--min-hits must be at least 1, got {min_hits}")
    if not 0 <= min_percent <= 100:
        raise ValueError(f"--min-percent must lie in 0 .. 100, got {min_percent}")
    if not 1 <= min_tables <= n_tables:
        raise ValueError(f"--min-tables must lie in 1 .. {n_tables} (the number of tables), got {min_tables}")


def decide(hits, n_valid, min_hits: int = 1, min_percent: int = 0, min_tables: int = 1):
    """The rule: (matched (R,) uint8, match (R, N) uint8) from hits (R, N) and n_valid (R,).  Exact: the products are formed in
    Python integers wherever 100 * hits or P * n_valid could leave 64 bits."""
    hits = np.asarray(hits)
    n_valid = np.asarray(n_valid)
    assert hits.ndim == 2 and n_valid.shape == (hits.shape[0],)
    validate_rule(min_hits, min_percent, min_tables, hits.shape[1])
    big = hits.size and (int(hits.max()) >= 2 ** 63 // 100 or int(n_valid.max()) >= 2 ** 63 // 100)
    h = hits.astype(object) if big else hits.astype(np.uint64)
    v = (n_valid.astype(object) if big else n_valid.astype(np.uint64))[:, None]
    match = (h >= min_hits) & (h * 100 >= v * int(min_percent)) & (v > 0)
    match = np.asarray(match, dtype=bool)
    matched = match.sum(axis=1) >= min_tables
    return matched.astype(np.uint8), match.astype(np.uint8)


def pair_flags(matched_1, matched_2, pair_rule: str = "any") -> np.ndarray:
    """One flag per pair from the two mates' flags: either (`any`) or both (`both`)."""
    if pair_rule not in PAIR_RULES:
        raise ValueError(f"--pair-rule must be one of {', '.join(PAIR_RULES)}, got {pair_rule!r}")
    a, b = np.asarray(matched_1) != 0, np.asarray(matched_2) != 0
    if a.shape != b.shape:
        raise ValueError(f"the two files of a pair must hold the same number of records: {a.size} and {b.size}")
    return ((a | b) if pair_rule == "any" else (a & b)).astype(np.uint8)


def starts_from(name_off, n_bytes: int) -> np.ndarray:
    """(R + 1,) uint64 record offsets from the records' name_off (the byte behind '>' or '@') and the stream's length."""
    return np.concatenate([np.asarray(name_off, dtype=np.uint64) - np.uint64(1), [np.uint64(n_bytes)]]).astype(np.uint64)


def record_starts(input_file: str, device: int = 0) -> np.ndarray:
    """(R + 1,) uint64: where every record of a FASTA / FASTQ file (by its name; plain, gzip or BGZF) begins in the
    decompressed stream -- its '>' or '@' -- and the stream's length.  One parse on the device, no tables: a counting indexer at
    k = 1, whose table is 4 bytes."""
    src = _Input(input_file, keep=False, quiet=True)
    n_bytes = 0
    with _lib.Indexer(1, device=device, fmt=src.fmt) as ix:
        for piece in src.pieces():
            ix.feed(piece)
            n_bytes += len(piece)
        recs = ix.records(ix.finish()["n_records"])
    return starts_from(recs["name_off"], n_bytes)


def select_records(input_file: str, keep, out_file, starts=None, device: int = 0) -> dict:
    """Writes the records of `input_file` whose flag in `keep` (R,) is set to `out_file` (through `.tmp` + rename), as the
    input's own bytes in file order; the flags may come from anywhere.  `starts`: record_starts(input_file), computed when
    not given.  Returns dict(n_records, n_kept, bytes_in, bytes_kept)."""
    keep = np.asarray(keep) != 0
    starts = record_starts(input_file, device) if starts is None else np.asarray(starts, dtype=np.uint64)
    if starts.shape != (keep.size + 1,):
        raise ValueError(f"{input_file} holds {starts.size - 1} records, and there are {keep.size} flags")
    src = _Input(input_file, keep=False, quiet=True)
    with _lib.Selector(device) as sel, atomic_write(out_file, "wb") as fhd:
        sel.set_records(starts, keep)
        for piece in src.pieces():
            fhd.write(memoryview(sel.feed(piece)))
        fin = sel.finish()
        select_s = sel.timings()["select_s"]
    if fin["bytes_fed"] != int(starts[-1]):
        raise ValueError(f"{input_file} changed between the passes: {fin['bytes_fed']} bytes now, {int(starts[-1])} when its records were found")
    return {"n_records": int(keep.size), "n_kept": int(keep.sum()), "bytes_in": fin["bytes_fed"], "bytes_kept": fin["bytes_kept"],
            "select_s": select_s}


def output_paths(project_name: str, query_file: str, mate: str = None, rest: bool = False) -> dict:
    """The sequence files of a run, by role: kept (and rest), with a mate kept_1, kept_2 (rest_1, rest_2); the extension is
    .fq for FASTQ input, .fa otherwise."""
    ext = "fq" if input_format(str(query_file)) == "fastq" else "fa"
    roles = [r + s for r in (["kept", "rest"] if rest else ["kept"]) for s in (["_1", "_2"] if mate else [""])]
    return {role: Path(f"{project_name}.{role}.{ext}") for role in roles}


def kmf_paths(project_name: str):
    return Path(f"{project_name}.kmf"), Path(f"{project_name}.kmf.json")


def filter_records(query_file: str, tables: Sequence, min_count: int = 1, max_count: int = 255, min_hits: int = 1, min_percent: int = 0,
                   min_tables: int = 1, invert: bool = False, mate: str = None, pair_rule: str = None, min_qual: int = 0, qual_offset: int = 33,
                   project_name: str = None, rest: bool = False, device: int = 0, hbm_budget: int = None, threads: int = DEFAULT_THREADS,
                   select=None, run=None, stage=None) -> dict:
    """The flags of every record of `query_file` (and of `mate`) under the rule, and with `project_name` the sequence files.

    Returns dict(keep (R,) uint8, match (R, N) uint8, hits (R, N), n_valid, seq_len (R,) uint64, names, kmer_len, lookup_s,
    starts (R + 1,), with a mate hits_2, n_valid_2, match_2, starts_2, and with `project_name` files: one dict per sequence
    file written (role, file, input, n_records, n_kept, bytes_in, bytes_kept)).
    `run` and `stage` go to query_records.  The record offsets come from a parse of their own (record_starts: the query's
    result says nothing about where a record lies in the stream) unless `run` reports name_off (R,) and n_bytes itself.  `select(input_file, keep, out_file, starts=, device=)` defaults to select_records (the CPU-only tests
    substitute all three)."""
    if pair_rule is not None and mate is None:
        raise ValueError("--pair-rule says how the two mates of a pair decide: it needs --mate")
    pair_rule = pair_rule or "any"
    if pair_rule not in PAIR_RULES:
        raise ValueError(f"--pair-rule must be one of {', '.join(PAIR_RULES)}, got {pair_rule!r}")
    validate_rule(min_hits, min_percent, min_tables, len(tables))
    if mate is not None and input_format(str(mate)) != input_format(str(query_file)):
        raise ValueError(f"the two files of a pair must have one format: {query_file} and {mate}")
    select = select or select_records
    tables = as_headers(tables, device)
    qual = {"min_qual": min_qual, "qual_offset": qual_offset} if min_qual else {}

    def phase1(path):
        res = query_records(str(path), tables, min_count, max_count, device=device, hbm_budget=hbm_budget, threads=threads, stage=stage, run=run,
                            **qual)
        matched, match = decide(res["hits"], res["n_valid"], min_hits, min_percent, min_tables)
        starts = starts_from(res["name_off"], res["n_bytes"]) if "name_off" in res and "n_bytes" in res else record_starts(str(path), device)
        return res, matched, match, starts

    res, matched, match, starts = phase1(query_file)
    out = {"match": match, "hits": np.asarray(res["hits"], dtype=np.uint64), "n_valid": np.asarray(res["n_valid"], dtype=np.uint64),
           "seq_len": np.asarray(res["seq_len"], dtype=np.uint64), "names": res.get("names", []), "kmer_len": res["kmer_len"], "starts": starts,
           "lookup_s": float(res.get("lookup_s", 0.0)), "n_groups": res.get("n_groups", 1), "min_count": min_count, "max_count": max_count}
    if mate is not None:
        res2, matched2, match2, starts2 = phase1(mate)
        if len(matched2) != len(matched):
            raise ValueError(f"the two files of a pair must hold the same number of records: {query_file} has {len(matched)}, {mate} has {len(matched2)}")
        matched = pair_flags(matched, matched2, pair_rule)
        out.update(hits_2=np.asarray(res2["hits"], dtype=np.uint64), n_valid_2=np.asarray(res2["n_valid"], dtype=np.uint64), match_2=match2,
                   starts_2=starts2, lookup_s=out["lookup_s"] + float(res2.get("lookup_s", 0.0)))
    keep = (matched == 0 if invert else matched != 0).astype(np.uint8)
    out["keep"] = keep
    out.update(_qual_keys(res))
    if project_name is not None:
        inputs = {"": (str(query_file), starts)} if mate is None else {"_1": (str(query_file), starts), "_2": (str(mate), out["starts_2"])}
        files, select_s = [], 0.0
        for role, path in output_paths(project_name, query_file, mate, rest).items():
            source, offs = inputs[role[4:]]
            flags = keep if role.startswith("kept") else 1 - keep
            done = select(source, flags, path, starts=offs, device=device)
            select_s += float(done.pop("select_s", 0.0))
            files.append({"role": role, "file": str(path), "input": source, **done})
            _mark(f"{path} written")
        out.update(files=files, select_s=select_s)
    return out


def filter(project_name: str, query_file: str, indexes: List[Path], min_count: int = 1, max_count: int = 255, min_hits: int = 1,   # noqa: A001
           min_percent: int = 0, min_tables: int = 1, invert: bool = False, rest: bool = False, mate: str = None, pair_rule: str = None,
           min_qual: int = None, qual_offset: int = None, device: int = 0, threads: int = DEFAULT_THREADS, hbm_budget: int = None,
           select=None, run=None, stage=None) -> dict:
    """The CLI's work: validate, query, decide, write the sequence files, `<project>.kmf` and `<project>.kmf.json`; returns
    filter_records' result.  Every refusal (ValueError) comes before any file is written; no file is overwritten."""
    qual_threshold(str(query_file), min_qual, qual_offset)
    if mate is not None:
        qual_threshold(str(mate), min_qual, qual_offset)
    if pair_rule is not None and mate is None:
        raise ValueError("--pair-rule says how the two mates of a pair decide: it needs --mate")
    if len(indexes) < 1:
        raise ValueError("a filter needs at least one table")
    validate_rule(min_hits, min_percent, min_tables, len(indexes))
    kmf, meta = kmf_paths(project_name)
    seq_paths = output_paths(project_name, query_file, mate, rest)
    refuse_files([kmf, meta] + list(seq_paths.values()), [query_file] + ([mate] if mate is not None else []))
    data, headers = verified_tables(indexes, min_count, max_count, device)
    extra = {"min_qual": min_qual, "qual_offset": 33 if qual_offset is None else qual_offset} if min_qual else {}
    result = filter_records(query_file, headers, min_count, max_count, min_hits, min_percent, min_tables, invert=invert, mate=mate,
                            pair_rule=pair_rule, project_name=project_name, rest=rest, device=device, hbm_budget=hbm_budget, threads=threads,
                            select=select, run=run, stage=stage, **extra)
    lean_headers(data)
    params = {"min_hits": int(min_hits), "min_percent": int(min_percent), "min_tables": int(min_tables), "invert": bool(invert),
              "pair_rule": (pair_rule or "any") if mate is not None else None}
    output = {"project_name": project_name, "kmer_len": int(result["kmer_len"]), "min_count": int(min_count), "max_count": int(max_count),
              "query_file": str(query_file), "data": data, **params, "mate_file": None if mate is None else str(mate),
              "n_records": int(result["keep"].size), "n_kept": int(result["keep"].sum()), "files": result["files"],
              "outputs": [f["file"] for f in result["files"]], "lookup_s": result["lookup_s"], "select_s": result["select_s"]}
    output.update(_qual_keys(result))
    write_json(meta, output)
    arrays = {"keep": result["keep"], "match": result["match"], "hits": result["hits"], "n_valid": result["n_valid"], "seq_len": result["seq_len"]}
    if mate is not None:
        arrays.update(hits_2=result["hits_2"], n_valid_2=result["n_valid_2"], match_2=result["match_2"])
    with atomic_write(kmf, "wb") as fhd:
        np.savez_compressed(fhd, **arrays, kmer_len=np.int64(result["kmer_len"]), min_count=np.int64(min_count), max_count=np.int64(max_count),
                            min_hits=np.int64(min_hits), min_percent=np.int64(min_percent), min_tables=np.int64(min_tables),
                            invert=np.bool_(invert), pair_rule=np.str_(params["pair_rule"] or ""))
    _mark("files renamed")
    return result


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Write the records of a FASTA/FASTQ file that match (or do not match) kmer databases.")
    parser.add_argument("Project_Name", metavar="P", type=str, help="Project name (prefix of the output files)")
    parser.add_argument("Query", metavar="Q", type=str, help="queries.fa|.fq[.gz|.bgz]")
    parser.add_argument("Kmer_N", metavar="K", type=Path, nargs="+", help="List of kin files")
    parser.add_argument("--min-count", type=int, default=1, help="Minimum Kmer Count [1]")
    parser.add_argument("--max-count", type=int, default=255, help="Maximum Kmer Count [255]")
    parser.add_argument("--min-hits", type=int, default=1, metavar="H", help="A table matches a record with at least H hits [1]")
    parser.add_argument("--min-percent", type=int, default=0, metavar="P", help="... and hits on at least P percent of its valid windows [0]")
    parser.add_argument("--min-tables", type=int, default=1, metavar="M", help="A record matches when at least M tables match it [1]")
    parser.add_argument("--invert", action="store_true", help="Keep the records that do not match (decontamination) [off]")
    parser.add_argument("--rest", action="store_true", help="Also write the records that are not kept, to <P>.rest.fa|.fq [off]")
    parser.add_argument("--mate", type=str, default=None, metavar="Q2", help="The second file of paired reads: record r of both files is one pair")
    parser.add_argument("--pair-rule", choices=PAIR_RULES, default=None, help="With --mate: a pair matches if any mate does, or both [any]")
    parser.add_argument("--threads", type=int, default=DEFAULT_THREADS, help=f"Host threads reading / inflating the tables [{DEFAULT_THREADS}]")
    parser.add_argument("--min-qual", type=int, default=None, metavar="Q", help="FASTQ: bases with a quality below Q count as N when matching [off]")
    parser.add_argument("--qual-offset", type=int, default=None, metavar="O", help="With --min-qual: the quality encoding, 33 or 64 [33]")
    return parser


def main(argv: List[str] = None) -> None:
    args = build_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    try:
        result = filter(args.Project_Name, args.Query, args.Kmer_N, min_count=args.min_count, max_count=args.max_count, min_hits=args.min_hits,
                        min_percent=args.min_percent, min_tables=args.min_tables, invert=args.invert, rest=args.rest, mate=args.mate,
                        pair_rule=args.pair_rule, min_qual=args.min_qual, qual_offset=args.qual_offset,
                        device=int(os.environ.get("PK_DEVICE", "0")), threads=args.threads)
    except ValueError as exc:
        print(f"error: {exc}", file=sys.stderr)
        sys.exit(1)
    kept = [f for f in result["files"] if f["role"].startswith("kept")]
    print(f"{int(result['keep'].sum())} of {result['keep'].size} records kept, {sum(f['bytes_kept'] for f in kept):,d} of "
          f"{sum(f['bytes_in'] for f in kept):,d} bytes, {' '.join(f['file'] for f in result['files'])}")
