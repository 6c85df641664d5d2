"""Trim host side: a FASTQ file and N `.kin[.bgz]` tables in, every read cut to its longest covered stretch out.

Positions, valid bases, valid windows, matching windows and covered bases are those of mask.py and query.py --coords,
applied to the FASTA text the FASTQ stands for (README "FASTQ input"); with `min_qual` a base below the threshold is an N:
not valid, never covered, the end of a run.  A RUN is a maximal stretch of consecutive positions of one read that all hold
covered bases -- the intervals of mask.py --bed.  The KEPT RUN of a read is its longest one, among equals the one with the
smallest start: trim_start, trim_end, half-open and 0-based, (0, 0) without a covered base.  A read is KEPT iff
trim_end - trim_start >= min_len (default kmer_len: exactly the reads with a matching window); with a mate file record r of
both files is one pair, kept iff both mates are.

Phase 1 (cover_bits) streams the reads against the staged tables with pk_query_set_cover, as mask.py does.  Phase 2
(trim_runs) streams them a second time through a _lib.Trimmer (pk_trim_*, kmer_trim.hip), cut into feeds of whole records:
where lines 2 and 4 of every record lie, and its kept run.  The decision is made on the host (decide).  Phase 3 needs no
kernel of its own: a trimmed read is a selection of byte ranges of its record, so every record is laid out as nine
consecutive segments (trim_segments) and filter.select_records writes the kept ones with pk_select as it stands.  No byte of
the output is ever changed, only left out; the output is not compressed.
The reference has no such tool; this is the khmer `filter-abund` / `bbduk ktrim` step.
"""
import argparse
import os
import sys
from pathlib import Path
from typing import List, Sequence

import numpy as np

from . import _lib
from .filter import record_starts, select_records, starts_from
from .indexer import _Input, _mark, input_format, qual_threshold
from .mask import or_cover
from .merger import DEFAULT_THREADS
from .output import atomic_write, write_json
from .query import _qual_keys, as_headers, plan_groups, refuse_files, stage_tables, stream_groups, validate, verified_tables
from .tables import lean_headers

TRIM_FEED = 64 << 20                # phase 2 reads this much at a time; a feed is the whole records of it and of the tail before it
GEOMETRY = ("pos2", "pos4", "end2", "end4", "lead")          # of _lib.TRIM_FIELDS: where lines 2 and 4 of a record lie
SEGMENT_FLAGS = (1, 0, 1, 0, 1, 0, 1, 0, 1)                  # header, cut, bases, cut, middle, cut, qualities, cut, tail


def check_fastq(reads_file: str) -> None:
    """FASTA input is refused: without qualities there is nothing to cut alongside, and mask.py marks its covered bases."""
    if input_format(str(reads_file)) != "fastq":
        raise ValueError(f"trim.py takes FASTQ input (.fq / .fastq[.gz|.bgz]): {reads_file} is FASTA by its name "
                         f"(mask.py marks the bases of a FASTA file that the tables cover)")


def validate_min_len(min_len) -> int:
    """L of `--min-len`: an integer >= 1 (a bool or a float is none)."""
    if isinstance(min_len, (bool, np.bool_)) or not isinstance(min_len, (int, np.integer)):
        raise ValueError(f"--min-len must be an integer, got {min_len!r}")
    if min_len < 1:
        raise ValueError(f"--min-len must be at least 1, got {min_len}")
    return int(min_len)


def run_cover(reads_file: str, kmer_len: int, ptrs, min_count: int, max_count: int, device: int = 0, first: bool = True,
              min_qual_byte: int = 0) -> dict:
    """mask.run_cover for FASTQ reads: one stream against the staged tables `ptrs` with the cover bits on, the bases below
    `min_qual_byte` counted as N.  Also hands back name_off (R,) and n_bytes, which give the record offsets without a parse of
    their own."""
    src = _Input(reads_file, keep=first, quiet=not first)
    n_bytes = 0
    with _lib.QueryIndexer(kmer_len, device=device, fmt=src.fmt, min_qual_byte=min_qual_byte) as q:
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
           "n_bases": n_bases, "n_bytes": n_bytes, "name_off": recs["name_off"].astype(np.uint64), "timings": timings}
    if first:
        out["names"] = [nm.decode("utf-8", "replace") for nm in src.names(recs)]
    return out


def cover_bits(reads_file: str, tables: Sequence, min_count: int = 1, max_count: int = 255, min_qual: int = 0, qual_offset: int = 33,
               device: int = 0, hbm_budget: int = None, threads: int = DEFAULT_THREADS, stage=None, run=None) -> dict:
    """mask.cover_bits for FASTQ reads (plain, gzip or BGZF): dict(names, seq_len, n_valid (R,), n_bases, cover, kmer_len,
    n_groups, lookup_s, and from run_cover name_off (R,) and n_bytes), the bits OR-ed over the table groups.  `run` receives
    min_qual_byte by keyword, and only when a threshold is set."""
    check_fastq(reads_file)
    extra = {"min_qual_byte": qual_threshold(str(reads_file), min_qual, qual_offset)} if min_qual else {}
    tables = as_headers(tables, device)
    kmer_len = validate(tables, min_count, max_count)
    result = stream_groups(reads_file, tables, kmer_len, plan_groups(tables, kmer_len, device, hbm_budget), min_count, max_count, run or run_cover,
                           or_cover, device, threads, stage or (lambda group, dev: stage_tables(group, dev, threads)), **extra)
    assert result["cover"].shape == ((result["n_bases"] + 7) // 8,)
    return result


class RecordFeeds:
    """The second pass over a FASTQ stream whose record offsets are known: iterating yields (piece, offsets) -- consecutive
    pieces of the stream, each the whole records of at most one block and of the tail carried from the block before, with
    the (n + 1,) offsets of its n records relative to the piece.  The bytes behind the last record (blank lines at most) come
    as pieces without a record, offsets = [their length].  `starts`: (R + 1,) record offsets (filter.record_starts).
    A record that ends in the block in which it begins or in the one behind it is fed whole, so a record of up to about two
    blocks is; ValueError when the carried tail and one further block still do not hold its end.  check(), after the loop,
    raises it if the stream is not the one the offsets were found in."""

    def __init__(self, reads_file: str, starts):
        self.reads_file = reads_file
        self.starts = np.ascontiguousarray(starts, dtype=np.uint64)
        self.R = self.starts.size - 1
        if self.starts.ndim != 1 or self.R < 0 or (self.R and int(self.starts[0]) != 0):
            raise ValueError(f"{reads_file}: the record offsets of a FASTQ stream begin at 0 and end with its length")
        self.block = min(TRIM_FEED, max(1 << 16, int(os.environ.get("PK_FEED_PIECE", TRIM_FEED))))
        self.pos, self.r, self.held = 0, 0, 0            # the stream offset of the carried tail = starts[r], the next record; its bytes

    def __iter__(self):
        starts, R, block = self.starts, self.R, self.block
        src = _Input(self.reads_file, keep=False, quiet=True)
        tail = np.zeros(0, dtype=np.uint8)
        for piece in src.pieces():
            view = np.frombuffer(piece, dtype=np.uint8)
            for off in range(0, view.size, block):
                buf = np.concatenate([tail, view[off:off + block]]) if tail.size else view[off:off + block]
                if self.r == R:                              # behind the last record (a stream of blank lines has none)
                    tail, self.held = tail[:0], 0
                    yield buf, np.array([buf.size], dtype=np.uint64)
                    self.pos += buf.size
                    continue
                hi = int(np.searchsorted(starts, self.pos + buf.size, side="right")) - 1   # records r .. hi - 1 lie whole in buf
                if hi <= self.r:
                    if buf.size > block:
                        raise ValueError(f"{self.reads_file}: record {self.r + 1} is longer than one feed of {block:,d} bytes")
                    tail = np.array(buf)
                    self.held = tail.size
                    continue
                cut = int(starts[hi]) - self.pos
                tail = np.array(buf[cut:])
                self.held = tail.size
                yield buf[:cut], starts[self.r:hi + 1] - np.uint64(self.pos)
                self.pos, self.r = self.pos + cut, hi

    def check(self) -> None:
        if self.r != self.R or self.held or self.pos != int(self.starts[-1]):
            raise ValueError(f"{self.reads_file} changed between the passes: {self.pos + self.held} bytes now, {int(self.starts[-1])} when its records "
                             f"were found")


def trim_runs(reads_file: str, cover, n_bases: int, starts, min_qual: int = 0, qual_offset: int = 33, device: int = 0) -> dict:
    """The kept run of every record of `reads_file` under the cover bits `cover` (packed as cover_bits returns them, for
    n_bases bases; the bits may come from anywhere).  `starts`: (R + 1,) record offsets (filter.record_starts).  The stream is
    re-cut at record offsets, the tail of a piece carried into the next (RecordFeeds).  Returns dict of the nine
    _lib.TRIM_FIELDS, (R,) uint64 each, and n_records, n_covered, trim_s.  ValueError if the carried tail and one further block of
    TRIM_FEED bytes do not hold the end of a record (one of up to about two blocks is fed whole), if `cover` does not hold
    n_bases bits or the file does not hold n_bases valid bases."""
    check_fastq(reads_file)
    bits = np.ascontiguousarray(cover, dtype=np.uint8)
    if bits.ndim != 1 or bits.size != (int(n_bases) + 7) // 8:
        raise ValueError(f"{int(n_bases)} bases take {(int(n_bases) + 7) // 8} bytes of cover bits, got an array of shape {bits.shape}")
    feeds = RecordFeeds(reads_file, starts)
    tq = qual_threshold(str(reads_file), min_qual, qual_offset) if min_qual else 0
    parts = []
    with _lib.Trimmer(device) as t:
        t.set_cover(bits, n_bases, tq)
        for piece, offsets in feeds:
            if offsets.size > 1:                             # the bytes behind the last record: no feed
                parts.append(t.feed(piece, offsets))
        try:
            fin = t.finish()
        except _lib.PkError as exc:
            if exc.code != _lib.PK_ERR_STATE:
                raise
            raise ValueError(f"{reads_file}: {exc}") from exc
        trim_s = t.timings()["trim_s"]
    feeds.check()
    out = {name: np.concatenate([p[name] for p in parts]) if parts else np.zeros(0, dtype=np.uint64) for name in _lib.TRIM_FIELDS}
    out.update(n_records=fin["n_records"], n_covered=fin["n_covered"], trim_s=trim_s)
    return out


def decide(trim_start, trim_end, min_len: int) -> np.ndarray:
    """keep (R,) uint8: read r is kept iff trim_end[r] - trim_start[r] >= min_len."""
    start, end = np.asarray(trim_start, dtype=np.uint64), np.asarray(trim_end, dtype=np.uint64)
    assert start.shape == end.shape and bool((start <= end).all())
    return (end - start >= np.uint64(validate_min_len(min_len))).astype(np.uint8)


def pair_keep(keep_1, keep_2) -> np.ndarray:
    """One flag per pair: kept iff both mates are.  ValueError if the two files differ in their number of records."""
    a, b = np.asarray(keep_1) != 0, np.asarray(keep_2) != 0
    if a.shape != b.shape:
        raise ValueError(f"the two files of a pair must hold the same number of records: {a.size} and {b.size}")
    return (a & b).astype(np.uint8)


def trim_segments(starts, geometry: dict, trim_start, trim_end, keep):
    """Every record as nine consecutive segments of its bytes -- header, cut, kept bases, cut, middle, cut, kept qualities,
    cut, tail -- with the flags 1, 0, 1, 0, 1, 0, 1, 0, 1 for a kept record and nine zeros for a dropped one:
    (offsets (9 R + 1,) uint64, non-decreasing, flags (9 R,) uint8), which select_records(..., starts=offsets) writes.
    `geometry`: the GEOMETRY fields of trim_runs.  The header is line 1 with its terminator; the middle is line 2's terminator
    and line 3 with its own; the tail is everything of the record behind line 4's content."""
    starts = np.asarray(starts, dtype=np.uint64)
    R = starts.size - 1
    ts, te = np.asarray(trim_start, dtype=np.uint64), np.asarray(trim_end, dtype=np.uint64)
    pos2, pos4, end2, end4, lead = (np.asarray(geometry[key], dtype=np.uint64) for key in GEOMETRY)
    cols = [starts[:-1], pos2 - lead, pos2 + ts, pos2 + te, end2, pos4 - lead, pos4 + ts, pos4 + te, end4]
    assert all(c.shape == (R,) for c in cols) and np.asarray(keep).shape == (R,)
    offsets = np.concatenate([np.stack(cols, axis=1).reshape(-1), starts[-1:]]).astype(np.uint64)
    if not bool((offsets[1:] >= offsets[:-1]).all()):
        at = int(np.flatnonzero(offsets[1:] < offsets[:-1])[0]) // 9
        raise ValueError(f"record {at + 1}: the lines of the record and its kept run do not lie in order")
    flags = ((np.asarray(keep) != 0)[:, None] & (np.array(SEGMENT_FLAGS, dtype=np.uint8) != 0)[None, :]).astype(np.uint8).reshape(-1)
    return offsets, flags


def output_paths(project_name: str, mate: str = None, rest: bool = False) -> dict:
    """The read files of a run, by role: trimmed (and rest), with a mate trimmed_1, trimmed_2 (rest_1, rest_2)."""
    roles = [r + s for r in (["trimmed", "rest"] if rest else ["trimmed"]) for s in (["_1", "_2"] if mate else [""])]
    return {role: Path(f"{project_name}.{role}.fq") for role in roles}


def kmt_paths(project_name: str):
    return Path(f"{project_name}.kmt"), Path(f"{project_name}.kmt.json")


def trim_records(reads_file: str, tables: Sequence, min_count: int = 1, max_count: int = 255, min_len: int = None, mate: str = None,
                 min_qual: int = 0, qual_offset: int = 33, project_name: str = None, rest: bool = False, device: int = 0, hbm_budget: int = None,
                 threads: int = DEFAULT_THREADS, stage=None, run=None, trim=None, select=None) -> dict:
    """The kept run and the flag of every record of `reads_file` (and of `mate`), and with `project_name` the read files.

    Returns dict(keep (R,) uint8, trim_start, trim_end, covered, seq_len, n_valid (R,) uint64, n_bases, starts (R + 1,),
    geometry, names, kmer_len, min_len, lookup_s, trim_s; with a mate the same arrays with `_2`, n_bases_2, starts_2 and
    geometry_2; with `project_name` select_s and files: one dict per read file written (role, file, input, n_records, n_kept,
    bytes_in, bytes_kept)).  `min_len`: None = kmer_len.
    `stage` and `run` go to cover_bits; `trim(reads_file, cover, n_bases, starts, min_qual=, qual_offset=, device=)` defaults
    to trim_runs and `select(input_file, keep, out_file, starts=, device=)` to filter.select_records (the CPU-only tests
    substitute all four).  The record offsets come from `run`'s name_off and n_bytes, else from a parse of their own."""
    check_fastq(reads_file)
    if mate is not None:
        check_fastq(mate)
    if min_len is not None:
        validate_min_len(min_len)
    tables = as_headers(tables, device)
    min_len = validate(tables, min_count, max_count) if min_len is None else int(min_len)
    qual = {"min_qual": min_qual, "qual_offset": qual_offset} if min_qual else {}

    def phases(path):
        res = cover_bits(str(path), tables, min_count, max_count, device=device, hbm_budget=hbm_budget, threads=threads, stage=stage, run=run, **qual)
        starts = starts_from(res["name_off"], res["n_bytes"]) if "name_off" in res and "n_bytes" in res else record_starts(str(path), device)
        done = (trim or trim_runs)(str(path), res["cover"], res["n_bases"], starts, device=device, **qual)
        if done["seq_len"].shape != res["seq_len"].shape or not np.array_equal(done["seq_len"], res["seq_len"]):
            raise ValueError(f"{path} changed between the passes: its records are not those that were looked up")
        _mark(f"{path} trimmed: {float(done.get('trim_s', 0.0)):.6f} s of HIP-event time in the trim kernels (lookup kernels: {res['lookup_s']:.6f} s)")
        return res, starts, done

    def arrays(res, starts, done, tag=""):
        out = {key + tag: np.asarray(done[key], dtype=np.uint64) for key in ("trim_start", "trim_end", "covered", "seq_len")}
        out.update({"n_valid" + tag: np.asarray(res["n_valid"], dtype=np.uint64), "n_bases" + tag: int(res["n_bases"]), "starts" + tag: starts,
                    "geometry" + tag: {key: done[key] for key in GEOMETRY}})
        return out

    res, starts, done = phases(reads_file)
    keep = decide(done["trim_start"], done["trim_end"], min_len)
    out = {**arrays(res, starts, done), "names": res.get("names", []), "kmer_len": res["kmer_len"], "min_len": min_len, "min_count": min_count,
           "max_count": max_count, "n_groups": res.get("n_groups", 1), "lookup_s": float(res.get("lookup_s", 0.0)), "trim_s": float(done.get("trim_s", 0.0))}
    if mate is not None:
        res2, starts2, done2 = phases(mate)
        if done2["trim_start"].shape != done["trim_start"].shape:
            raise ValueError(f"the two files of a pair must hold the same number of records: {reads_file} has {keep.size}, "
                             f"{mate} has {done2['trim_start'].size}")
        keep = pair_keep(keep, decide(done2["trim_start"], done2["trim_end"], min_len))
        out.update(arrays(res2, starts2, done2, "_2"), lookup_s=out["lookup_s"] + float(res2.get("lookup_s", 0.0)),
                   trim_s=out["trim_s"] + float(done2.get("trim_s", 0.0)))
    out["keep"] = keep
    if min_qual:
        out.update(min_qual=int(min_qual), qual_offset=int(qual_offset))
    if project_name is not None:
        select = select or select_records
        tags = {"": (str(reads_file), "")} if mate is None else {"_1": (str(reads_file), ""), "_2": (str(mate), "_2")}
        files, select_s = [], 0.0
        for role, path in output_paths(project_name, mate, rest).items():
            source, tag = tags[role[-2:] if mate is not None else ""]
            if role.startswith("trimmed"):
                offsets, flags = trim_segments(out["starts" + tag], out["geometry" + tag], out["trim_start" + tag], out["trim_end" + tag], keep)
                done = select(source, flags, path, starts=offsets, device=device)
                kept = keep
            else:
                done = select(source, 1 - keep, path, starts=out["starts" + tag], device=device)
                kept = 1 - keep
            select_s += float(done.pop("select_s", 0.0))
            files.append({"role": role, "file": str(path), "input": source, **done, "n_records": int(keep.size), "n_kept": int(kept.sum())})
            _mark(f"{path} written")
        out.update(files=files, select_s=select_s)
    return out


def summary(result: dict) -> dict:
    """The counts of a trim_records result: n_records, n_kept, n_trimmed (kept records -- with a mate: pairs -- of which a
    read is shorter than it was), bases_in (the positions of all reads) and bases_kept (those of the kept runs of the kept reads)."""
    keep = result["keep"] != 0
    cut = np.zeros(keep.size, dtype=bool)
    bases_in = bases_kept = 0
    for tag in ("", "_2") if "trim_start_2" in result else ("",):
        length = result["trim_end" + tag] - result["trim_start" + tag]
        cut |= length < result["seq_len" + tag]
        bases_in += int(result["seq_len" + tag].sum())
        bases_kept += int(length[keep].sum())
    return {"n_records": int(keep.size), "n_kept": int(keep.sum()), "n_trimmed": int((keep & cut).sum()), "bases_in": bases_in, "bases_kept": bases_kept}


def trim(project_name: str, reads_file: str, indexes: List[Path], min_count: int = 1, max_count: int = 255, min_len: int = None,   # noqa: A001
         mate: str = None, rest: bool = False, min_qual: int = None, qual_offset: int = None, device: int = 0, threads: int = DEFAULT_THREADS,
         hbm_budget: int = None, stage=None, run=None, trim=None, select=None) -> dict:
    """The CLI's work: validate, look up, trim, decide, write the read files, `<project>.kmt` and `<project>.kmt.json`; returns
    trim_records' result with summary()'s counts.  Every refusal (ValueError) comes before any file is written; no file is
    overwritten."""
    check_fastq(reads_file)
    qual_threshold(str(reads_file), min_qual, qual_offset)
    if mate is not None:
        check_fastq(mate)
        qual_threshold(str(mate), min_qual, qual_offset)
    if min_len is not None:
        validate_min_len(min_len)
    if len(indexes) < 1:
        raise ValueError("a trim needs at least one table")
    kmt, meta = kmt_paths(project_name)
    refuse_files([kmt, meta] + list(output_paths(project_name, mate, rest).values()), [reads_file] + ([mate] if mate is not None else []))
    data, headers = verified_tables(indexes, min_count, max_count, device)
    extra = {"min_qual": min_qual, "qual_offset": 33 if qual_offset is None else qual_offset} if min_qual else {}
    result = trim_records(reads_file, headers, min_count, max_count, min_len=min_len, mate=mate, project_name=project_name, rest=rest,
                          device=device, hbm_budget=hbm_budget, threads=threads, stage=stage, run=run, trim=trim, select=select, **extra)
    result.update(summary(result))
    lean_headers(data)
    output = {"project_name": project_name, "kmer_len": int(result["kmer_len"]), "min_count": int(min_count), "max_count": int(max_count),
              "query_file": str(reads_file), "data": data, "min_len": int(result["min_len"]), "mate_file": None if mate is None else str(mate),
              **{key: result[key] for key in ("n_records", "n_kept", "n_trimmed", "bases_in", "bases_kept")}, "files": result["files"],
              "outputs": [f["file"] for f in result["files"]], "lookup_s": result["lookup_s"], "trim_s": result["trim_s"],
              "select_s": result["select_s"]}
    output.update(_qual_keys(result))
    write_json(meta, output)
    names = ("trim_start", "trim_end", "covered", "seq_len", "n_valid")
    arrays = {key + tag: np.ascontiguousarray(result[key + tag], dtype=np.uint64) for tag in (("", "_2") if mate is not None else ("",)) for key in names}
    if mate is not None:
        arrays["n_bases_2"] = np.uint64(result["n_bases_2"])
    with atomic_write(kmt, "wb") as fhd:
        np.savez_compressed(fhd, **arrays, keep=np.ascontiguousarray(result["keep"], dtype=np.uint8), kmer_len=np.int64(result["kmer_len"]),
                            min_count=np.int64(min_count), max_count=np.int64(max_count), min_len=np.int64(result["min_len"]),
                            n_bases=np.uint64(result["n_bases"]))
    _mark("files renamed")
    return result


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Trim the reads of a FASTQ file to the longest stretch that kmer databases cover.")
    parser.add_argument("Project_Name", metavar="P", type=str, help="Project name (prefix of the output files)")
    parser.add_argument("Reads", metavar="Q", type=str, help="reads.fq[.gz|.bgz]")
    parser.add_argument("Kmer_N", metavar="K", type=Path, nargs="+", help="List of kin files")
    parser.add_argument("--min-count", type=int, default=1, help="Minimum Kmer Count [1]")
    parser.add_argument("--max-count", type=int, default=255, help="Maximum Kmer Count [255]")
    parser.add_argument("--min-len", type=int, default=None, metavar="L", help="Keep the reads whose kept run is at least L bases long [kmer_len]")
    parser.add_argument("--mate", type=str, default=None, metavar="Q2", help="The second file of paired reads: record r of both files is one pair, kept iff both mates are")
    parser.add_argument("--rest", action="store_true", help="Also write the reads that are not kept, untrimmed, to <P>.rest.fq [off]")
    parser.add_argument("--min-qual", type=int, default=None, metavar="Q", help="Bases with a quality below Q count as N: they end a run [off]")
    parser.add_argument("--qual-offset", type=int, default=None, metavar="O", help="With --min-qual: the quality encoding, 33 or 64 [33]")
    parser.add_argument("--threads", type=int, default=DEFAULT_THREADS, help=f"Host threads reading / inflating the tables [{DEFAULT_THREADS}]")
    return parser


def main(argv: List[str] = None) -> None:
    args = build_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    try:
        result = trim(args.Project_Name, args.Reads, args.Kmer_N, min_count=args.min_count, max_count=args.max_count, min_len=args.min_len,
                      mate=args.mate, rest=args.rest, min_qual=args.min_qual, qual_offset=args.qual_offset,
                      device=int(os.environ.get("PK_DEVICE", "0")), threads=args.threads)
    except ValueError as exc:
        print(f"error: {exc}", file=sys.stderr)
        sys.exit(1)
    what = "pairs" if args.mate else "reads"
    print(f"{result['n_kept']} of {result['n_records']} {what} kept, {result['n_trimmed']} of them trimmed, {result['bases_kept']:,d} of "
          f"{result['bases_in']:,d} bases, {' '.join(f['file'] for f in result['files'])}")
