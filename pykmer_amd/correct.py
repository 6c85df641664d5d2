"""Correct host side: a FASTQ file and N `.kin[.bgz]` tables in, the same file with its single-base errors put back out.

Positions, valid bases, valid windows, matching windows and covered bases are those of trim.py (README "Trimming reads"),
and so are --min-count, --max-count, --min-qual and --qual-offset: with `min_qual` a base below the threshold is an N, not
valid, never a candidate, the end of a run.  A VALID RUN is a maximal stretch [lo, hi) of consecutive positions of one read
that all hold valid bases; window s is the positions [s, s + k).  A CANDIDATE is a position p that holds a valid base, is not
covered and lies in a valid run with hi - lo >= k; its windows are W(p) = {s : max(lo, p - k + 1) <= s <= min(p, hi - k)},
w(p) of them.  It is TRIED iff w(p) >= min_windows (default (kmer_len + 1) // 2).  A base b other than the read's own PASSES
iff every window of W(p) matches when read with b at p and the read's own bases everywhere else.  The candidate is CORRECTED
iff exactly one base passes, AMBIGUOUS iff two or three do, UNFIXABLE iff none does.  Every candidate is judged against the
uncorrected read.  A corrected byte becomes "ACGT"[b] | (old & 0x20); no other byte of the file changes.

All tables are staged as ONE group, once, and serve both passes: trim.run_cover for the cover bits, then a _lib.Corrector
(pk_correct_*, kmer_correct.hip) on the same pointers, the stream re-cut at record offsets by trim.RecordFeeds.
The reference has no such tool; this is the step of Musket, Lighter, BFC and `bbduk` / tadpole `ecc`.
"""
import argparse
import os
import sys
from pathlib import Path
from typing import List, Sequence

import numpy as np

from . import _lib
from .filter import record_starts, starts_from
from .indexer import _mark, input_format, qual_threshold
from .merger import DEFAULT_THREADS
from .output import atomic_write, write_json
from .query import _qual_keys, as_headers, plan_groups, refuse_files, stage_tables, stream_groups, validate, verified_tables
from .tables import lean_headers
from .trim import RecordFeeds, run_cover

COUNTS = ("candidates", "untried", "corrected", "ambiguous")
MAX_TABLES = 16                     # pk_correct_set_tables: one launch reads them all


def check_fastq(reads_file: str) -> None:
    """FASTA input is refused, as trim.py refuses it: the output is the input's records, line 4 included."""
    if input_format(str(reads_file)) != "fastq":
        raise ValueError(f"correct.py takes FASTQ input (.fq / .fastq[.gz|.bgz]): {reads_file} is FASTA by its name")


def validate_min_windows(min_windows, kmer_len: int) -> int:
    """M of `--min-windows`: an integer 1 <= M <= kmer_len (a bool or a float is none); None = (kmer_len + 1) // 2."""
    if min_windows is None:
        return (int(kmer_len) + 1) // 2
    if isinstance(min_windows, (bool, np.bool_)) or not isinstance(min_windows, (int, np.integer)):
        raise ValueError(f"--min-windows must be an integer, got {min_windows!r}")
    if not 1 <= min_windows <= kmer_len:
        raise ValueError(f"--min-windows must lie in 1 .. kmer_len = {kmer_len}, got {min_windows}")
    return int(min_windows)


def fixes_from(original, patched, starts, pos2, corrected=None):
    """(fix_record, fix_pos (F,) uint64, fix_old, fix_new (F,) uint8), in stream order, from the bytes in which `patched`
    differs from `original`: the record of the byte at offset d is the one whose [starts[r], starts[r + 1]) holds it, and
    fix_pos = d - pos2[r].  `starts` and `pos2` are offsets into the two texts.  ValueError if the texts differ in length,
    if a byte in front of a record's position 0 differs, or -- with `corrected` (R,) -- if corrected.sum() is not F."""
    a, b = np.frombuffer(original, dtype=np.uint8), np.frombuffer(patched, dtype=np.uint8)
    starts, pos2 = np.asarray(starts, dtype=np.uint64), np.asarray(pos2, dtype=np.uint64)
    if a.shape != b.shape:
        raise ValueError(f"the corrected text holds {b.size} bytes, the text it was made from {a.size}")
    at = np.flatnonzero(a != b).astype(np.uint64)
    rec = (np.searchsorted(starts, at, side="right") - 1).astype(np.int64)
    if at.size and (rec.min() < 0 or rec.max() >= pos2.size or bool((at < pos2[rec]).any())):
        raise ValueError("a byte outside the positions of a record differs between the text and its corrected copy")
    if corrected is not None and int(np.asarray(corrected, dtype=np.uint64).sum()) != at.size:
        raise ValueError(f"{int(np.asarray(corrected, dtype=np.uint64).sum())} positions were corrected, {at.size} bytes differ")
    return rec.astype(np.uint64), at - pos2[rec] if at.size else at, a[at.astype(np.int64)].copy(), b[at.astype(np.int64)].copy()


def correct_runs(reads_file: str, cover, n_bases: int, starts, ptrs, kmer_len: int, min_count: int = 1, max_count: int = 255,
                 min_windows: int = None, min_qual: int = 0, qual_offset: int = 33, out_file=None, device: int = 0) -> dict:
    """The corrections of every record of `reads_file` under the cover bits `cover` (packed as trim.cover_bits returns them,
    for n_bases bases; the bits may come from anywhere) against the staged tables `ptrs`.  `starts`: (R + 1,) record offsets.
    With `out_file` the corrected text is written there (`.tmp` + rename).  Returns dict of the six _lib.CORR_FIELDS, (R,)
    uint64 each, fix_record, fix_pos, fix_old, fix_new (fixes_from), n_records, n_bases, n_candidates, n_untried, n_corrected,
    n_ambiguous, bytes and correct_s.  ValueError as trim.trim_runs raises it."""
    check_fastq(reads_file)
    bits = np.ascontiguousarray(cover, dtype=np.uint8)
    if bits.ndim != 1 or bits.size != (int(n_bases) + 7) // 8:
        raise ValueError(f"{int(n_bases)} bases take {(int(n_bases) + 7) // 8} bytes of cover bits, got an array of shape {bits.shape}")
    M = validate_min_windows(min_windows, kmer_len)
    feeds = RecordFeeds(reads_file, starts)
    tq = qual_threshold(str(reads_file), min_qual, qual_offset) if min_qual else 0
    parts, fixes = [], []

    def run(sink):
        done, n_bytes = 0, 0
        with _lib.Corrector(kmer_len, device) as c:
            c.set_tables(ptrs, min_count, max_count)
            c.set_cover(bits, n_bases, tq, M)
            for piece, offsets in feeds:
                if offsets.size > 1:
                    fields, patched = c.feed(piece, offsets)
                    rec, pos, old, new = fixes_from(piece, patched, offsets, fields["pos2"] - np.uint64(n_bytes), fields["corrected"])
                    parts.append(fields)
                    fixes.append((rec + np.uint64(done), pos, old, new))
                    done += offsets.size - 1
                else:
                    patched = piece                          # behind the last record: blank lines, as they are
                if sink is not None:
                    sink.write(patched.tobytes())
                n_bytes += piece.size
            try:
                fin = c.finish()
            except _lib.PkError as exc:
                if exc.code != _lib.PK_ERR_STATE:
                    raise
                raise ValueError(f"{reads_file}: {exc}") from exc
            fin.update(correct_s=c.timings()["correct_s"], bytes=n_bytes)
        feeds.check()
        return fin

    if out_file is None:
        fin = run(None)
    else:
        with atomic_write(out_file, "wb") as fhd:
            fin = run(fhd)
    out = {name: np.concatenate([p[name] for p in parts]) if parts else np.zeros(0, dtype=np.uint64) for name in _lib.CORR_FIELDS}
    for i, (name, dtype) in enumerate((("fix_record", np.uint64), ("fix_pos", np.uint64), ("fix_old", np.uint8), ("fix_new", np.uint8))):
        out[name] = np.concatenate([f[i] for f in fixes]).astype(dtype) if fixes else np.zeros(0, dtype=dtype)
    out.update(fin)
    return out


def output_path(project_name: str) -> Path:
    return Path(f"{project_name}.corrected.fq")


def kme_paths(project_name: str):
    return Path(f"{project_name}.kme"), Path(f"{project_name}.kme.json")


def correct_records(reads_file: str, tables: Sequence, min_count: int = 1, max_count: int = 255, min_windows: int = None, min_qual: int = 0,
                    qual_offset: int = 33, project_name: str = None, device: int = 0, hbm_budget: int = None, threads: int = DEFAULT_THREADS,
                    stage=None, run=None, correct=None) -> dict:
    """The corrections of every record of `reads_file`, and with `project_name` the corrected file.

    Returns dict(candidates, untried, corrected, ambiguous, unfixable, seq_len, n_valid (R,) uint64, fix_record, fix_pos,
    fix_old, fix_new, n_bases, names, kmer_len, min_count, max_count, min_windows, bytes, lookup_s, correct_s; with
    `project_name` output, the file written).  The tables are staged once, as one group (ValueError if the HBM budget holds
    fewer, or for more than 16), and serve both passes.  `stage` and `run` are trim.cover_bits' hooks;
    `correct(reads_file, cover, n_bases, starts, ptrs, kmer_len, min_count, max_count, min_windows=, out_file=, device=,
    [min_qual=, qual_offset=])` defaults to correct_runs (the CPU-only tests substitute all three)."""
    check_fastq(reads_file)
    extra = {"min_qual_byte": qual_threshold(str(reads_file), min_qual, qual_offset)} if min_qual else {}
    qual = {"min_qual": min_qual, "qual_offset": qual_offset} if min_qual else {}
    tables = as_headers(tables, device)
    kmer_len = validate(tables, min_count, max_count)
    M = validate_min_windows(min_windows, kmer_len)
    if len(tables) > MAX_TABLES:
        raise ValueError(f"a correction takes at most {MAX_TABLES} tables, all in one lookup; got {len(tables)}")
    groups = plan_groups(tables, kmer_len, device, hbm_budget)
    if len(groups) > 1:
        raise ValueError(f"a correction needs all {len(tables)} tables of {4 ** kmer_len:,d} bytes staged together, and the HBM budget holds "
                         f"{groups[0][1]} at a time: take fewer tables or a larger budget (PK_MERGE_HBM_BUDGET)")
    out_file = None if project_name is None else output_path(project_name)

    def both(path, k, ptrs, mn, mx, dev, first, **kw):
        """The two passes against one staging: the cover bits, then the corrections on the same pointers."""
        res = (run or run_cover)(path, k, ptrs, mn, mx, dev, first, **kw)
        starts = starts_from(res["name_off"], res["n_bytes"]) if "name_off" in res and "n_bytes" in res else record_starts(str(path), dev)
        done = (correct or correct_runs)(str(path), res["cover"], res["n_bases"], starts, ptrs, k, mn, mx, min_windows=M, out_file=out_file,
                                         device=dev, **qual)
        if done["seq_len"].shape != res["seq_len"].shape or not np.array_equal(done["seq_len"], res["seq_len"]):
            raise ValueError(f"{path} changed between the passes: its records are not those that were looked up")
        res["done"] = done
        return res

    res = stream_groups(str(reads_file), tables, kmer_len, groups, min_count, max_count, both, lambda result, part: part, device, threads,
                        stage or (lambda group, dev: stage_tables(group, dev, threads)), **extra)
    done = res.pop("done")
    _mark(f"{reads_file} corrected: {float(done.get('correct_s', 0.0)):.6f} s of HIP-event time in the correct kernels (lookup kernels: {res['lookup_s']:.6f} s)")
    out = {key: np.asarray(done[key], dtype=np.uint64) for key in COUNTS + ("seq_len", "fix_record", "fix_pos")}
    out["unfixable"] = out["candidates"] - out["untried"] - out["corrected"] - out["ambiguous"]
    out.update(fix_old=np.asarray(done["fix_old"], dtype=np.uint8), fix_new=np.asarray(done["fix_new"], dtype=np.uint8),
               n_valid=np.asarray(res["n_valid"], dtype=np.uint64), n_bases=int(res["n_bases"]), names=res.get("names", []), kmer_len=kmer_len,
               min_count=min_count, max_count=max_count, min_windows=M, bytes=int(done.get("bytes", res.get("n_bytes", 0))),
               lookup_s=float(res.get("lookup_s", 0.0)), correct_s=float(done.get("correct_s", 0.0)))
    if int(out["corrected"].sum()) != out["fix_record"].size:
        raise ValueError(f"{int(out['corrected'].sum())} positions were corrected, {out['fix_record'].size} bytes differ")
    if min_qual:
        out.update(min_qual=int(min_qual), qual_offset=int(qual_offset))
    if out_file is not None:
        out["output"] = str(out_file)
    return out


def summary(result: dict) -> dict:
    """The counts of a correct_records result."""
    out = {"n_records": int(result["seq_len"].size), "n_reads_corrected": int((result["corrected"] > 0).sum())}
    out.update({"n_" + key: int(result[key].sum()) for key in COUNTS + ("unfixable",)})
    return out


def correct(project_name: str, reads_file: str, indexes: List[Path], min_count: int = 1, max_count: int = 255, min_windows: int = None,
            min_qual: int = None, qual_offset: int = None, device: int = 0, threads: int = DEFAULT_THREADS, hbm_budget: int = None, stage=None,
            run=None, correct=None) -> dict:   # noqa: A002
    """The CLI's work: validate, look up, correct, write `<project>.corrected.fq`, `<project>.kme` and `<project>.kme.json`;
    returns correct_records' result with summary()'s counts.  Every refusal (ValueError) comes before any file is written; no
    file is overwritten."""
    check_fastq(reads_file)
    qual_threshold(str(reads_file), min_qual, qual_offset)
    if len(indexes) < 1:
        raise ValueError("a correction needs at least one table")
    kme, meta = kme_paths(project_name)
    refuse_files([kme, meta, output_path(project_name)], [reads_file])
    data, headers = verified_tables(indexes, min_count, max_count, device)
    validate_min_windows(min_windows, validate(headers, min_count, max_count))
    extra = {"min_qual": min_qual, "qual_offset": 33 if qual_offset is None else qual_offset} if min_qual else {}
    result = correct_records(reads_file, headers, min_count, max_count, min_windows=min_windows, project_name=project_name, device=device,
                             hbm_budget=hbm_budget, threads=threads, stage=stage, run=run, correct=correct, **extra)
    result.update(summary(result))
    lean_headers(data)
    output = {"project_name": project_name, "kmer_len": int(result["kmer_len"]), "min_count": int(min_count), "max_count": int(max_count),
              "query_file": str(reads_file), "data": data, "min_windows": int(result["min_windows"]),
              **{key: result[key] for key in ("n_records", "n_candidates", "n_untried", "n_corrected", "n_ambiguous", "n_unfixable", "n_reads_corrected")},
              "bytes": int(result["bytes"]), "output": result["output"], "lookup_s": result["lookup_s"], "correct_s": result["correct_s"]}
    output.update(_qual_keys(result))
    write_json(meta, output)
    with atomic_write(kme, "wb") as fhd:
        np.savez_compressed(fhd, **{key: np.ascontiguousarray(result[key], dtype=np.uint64) for key in COUNTS + ("seq_len", "n_valid", "fix_record", "fix_pos")},
                            fix_old=np.ascontiguousarray(result["fix_old"], dtype=np.uint8), fix_new=np.ascontiguousarray(result["fix_new"], dtype=np.uint8),
                            kmer_len=np.int64(result["kmer_len"]), min_count=np.int64(min_count), max_count=np.int64(max_count),
                            min_windows=np.int64(result["min_windows"]), n_bases=np.uint64(result["n_bases"]))
    _mark("files renamed")
    return result


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Correct single-base errors in the reads of a FASTQ file from the kmers of kmer databases.")
    parser.add_argument("Project_Name", metavar="P", type=str, help="Project name (prefix of the output files)")
    parser.add_argument("Reads", metavar="Q", type=str, help="reads.fq[.gz|.bgz]")
    parser.add_argument("Kmer_N", metavar="K", type=Path, nargs="+", help="List of kin files")
    parser.add_argument("--min-count", type=int, default=1, help="Minimum Kmer Count [1]")
    parser.add_argument("--max-count", type=int, default=255, help="Maximum Kmer Count [255]")
    parser.add_argument("--min-windows", type=int, default=None, metavar="M", help="Try a base only when at least M windows hold it [(kmer_len + 1) // 2]")
    parser.add_argument("--min-qual", type=int, default=None, metavar="Q", help="Bases with a quality below Q count as N: never corrected, they end a run [off]")
    parser.add_argument("--qual-offset", type=int, default=None, metavar="O", help="With --min-qual: the quality encoding, 33 or 64 [33]")
    parser.add_argument("--threads", type=int, default=DEFAULT_THREADS, help=f"Host threads reading / inflating the tables [{DEFAULT_THREADS}]")
    return parser


def main(argv: List[str] = None) -> None:
    args = build_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    try:
        result = correct(args.Project_Name, args.Reads, args.Kmer_N, min_count=args.min_count, max_count=args.max_count,
                         min_windows=args.min_windows, min_qual=args.min_qual, qual_offset=args.qual_offset,
                         device=int(os.environ.get("PK_DEVICE", "0")), threads=args.threads)
    except ValueError as exc:
        print(f"error: {exc}", file=sys.stderr)
        sys.exit(1)
    print(f"{result['n_corrected']} bases corrected in {result['n_reads_corrected']} of {result['n_records']} reads "
          f"({result['n_candidates']} candidates: {result['n_untried']} untried, {result['n_ambiguous']} ambiguous, {result['n_unfixable']} unfixable), "
          f"{result['output']}")
