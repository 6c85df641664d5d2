"""Unitigs host side: ONE `.kin[.bgz]` table in, the compacted de Bruijn graph of its k-mers out as FASTA.

Input: one table T of 4^k bytes, k odd, 1 <= k <= 17, and a count window 1 <= min <= max <= 255.  Any combination of tables
is a table made first with `extract.py --table`.
    Node.  A canonical address x with min <= T[x] <= max.  S is the node set and n_nodes = |S|.
    Oriented k-mer.  Any value o in [0, 4^k), codes A,C,G,T = 0..3, first base in the highest bits.  rc(o) is its reverse
        complement and canon(o) = min(o, rc(o)).  k is odd, so o != rc(o) always.
    Edges.  out(o) = { t = ((o << 2) | b) & (4^k - 1), b = 0..3 : canon(t) in S }; in(t) = { rc(u) : u in out(rc(t)) }.  Edges
        are counted as strings: two successors that are each other's reverse complement count as two.
    Compactable edge.  o -> t is compactable iff |out(o)| = 1, |in(t)| = 1 and canon(o) != canon(t).  Self-loops such as
        poly-A, and hairpins o -> rc(o), count in the degrees but are never compacted.  Compactable edges are symmetric, so
        they form a matching on (node, side), and every component is a simple path or a simple cycle that meets each node once.
    Unitig.  A maximal sequence o_1 -> ... -> o_n of compactable edges, n >= 1.  Every node lies in exactly one unitig.  Its
        text is the k letters of o_1 followed by the last letter of each o_i, i >= 2.  Its length is L = n + k - 1.
    Orientation and order.  A linear unitig, n >= 2, is spelled starting from the end node with the smaller canonical
        address, leaving that node towards the rest; first_addr is that address.  A single node is spelled as its canonical
        k-mer.  A cycle (circular = 1) starts at its smallest canonical address x_min, spelled forward from the canonical
        string of x_min, and stops before returning to it; its last k - 1 letters overlap its start.  Rows are all linear
        unitigs by ascending first_addr, then all circular ones by ascending first_addr.
    Per unitig.  n_kmers = n; depth = the sum of T[x] over its nodes; circular.
    min_kmers M.  Unitigs with n_kmers < M are not written and get no row; n_short counts them, nodes_short their nodes.
    A branching node has |out(o)| >= 2 for o = x or o = rc(x).
    The graph (gfa=True, --gfa).  A written row r with the path o_1 -> ... -> o_n has the oriented rows (r,+), tail o_1 and head
        o_n, and (r,-), tail rc(o_n) and head rc(o_1).  (r,s) -> (q,u) is an edge iff tail(q,u) in out(head(r,s)); the overlap
        is k - 1 bases.  Edges are ordered by from row, + before -, then the successor's base; an edge and its mirror
        (q,~u) -> (r,~s) are both written, an edge that is its own mirror once; edges into unitigs that min_kmers dropped are
        counted (edges_dropped), not written.  README "Unitigs" has the whole of it.

The table is staged whole in HBM (staging.staged_pieces) beside a link array of the same size; pk_unitig_build (kmer_unitig.hip)
finds the links, walks the paths and the cycles and writes the whole FASTA on the device -- `>` + the row index + newline + the
text + newline per row --, which comes back in slices.  The reference has no such tool; this is the BCALM step.  One device.
"""
import argparse
import os
import sys
from pathlib import Path
from typing import List

import numpy as np

from . import _lib, staging
from .extract import _kmer_len_of
from .indexer import _mark
from .merger import DEFAULT_THREADS
from .output import atomic_write, write_json
from .query import as_headers, load_header, refuse_files
from .tables import common_kmer_len, lean_headers, name_of, table_entry

TEXT_SLICE = 64 << 20               # the FASTA comes back from the device this many bytes at a time
COMBINE = "combine several tables into one first: extract.py <project> --present a.kin b.kin ... --table max"


def check_window(min_count: int, max_count: int, min_kmers) -> None:
    if not 1 <= min_count <= max_count <= 255:
        raise ValueError(f"the count window must satisfy 1 <= min <= max <= 255, got {min_count}-{max_count}")
    if isinstance(min_kmers, (bool, np.bool_)) or not isinstance(min_kmers, (int, np.integer)) or not 1 <= int(min_kmers) < 2 ** 63:
        raise ValueError(f"--min-kmers must be an integer >= 1, got {min_kmers!r}")


def validate(tables, min_count: int = 1, max_count: int = 255, min_kmers: int = 1) -> int:
    """The checks that need no device; returns kmer_len.  ValueError for anything but one table of an odd kmer_len <= 17, a
    window outside 1 <= min <= max <= 255 and an M that is no integer >= 1."""
    if len(tables) != 1:
        raise ValueError(f"unitigs are built from exactly one table, got {len(tables)}: {COMBINE}")
    check_window(min_count, max_count, min_kmers)
    return common_kmer_len(tables, "unitigs", _kmer_len_of)


def n50(lengths) -> int:
    """The N50 of the lengths: the largest L such that the sequences of length >= L hold at least half of all bases; 0 for none."""
    lengths = np.sort(np.asarray(lengths, dtype=np.uint64))[::-1]
    if lengths.size == 0:
        return 0
    run = np.cumsum(lengths, dtype=np.uint64)
    return int(lengths[int(np.searchsorted(run, (int(run[-1]) + 1) // 2))])


def check_budget(table, kmer_len: int, device: int, hbm_budget: int = None) -> None:
    """A table that is staged needs 2 * 4^k bytes of the HBM budget (itself and the link array), a resident one 4^k; refused
    here, before anything is staged."""
    resident = hasattr(table, "device_slice")
    need = (1 if resident else 2) * 4 ** kmer_len
    budget = staging.hbm_budget(device, hbm_budget)
    if need > budget:
        raise ValueError(f"the table and its link array take {need} bytes, the HBM budget is {budget} (PK_MERGE_HBM_BUDGET)")


def stage_table(table, kmer_len: int, device: int, threads: int):
    """(device pointer of the whole table, free()): staged by staging.staged_pieces, or used where it lies."""
    if hasattr(table, "device_slice") and (table.first != 0 or table.n != 4 ** kmer_len):
        raise ValueError("unitigs need the whole table resident, not a slice of it")
    pieces = staging.staged_pieces([table], [(0, 4 ** kmer_len)], device, threads)
    ptrs, _, _ = next(pieces)
    return ptrs[0], pieces.close


def run_build(ptr, kmer_len: int, min_count: int, max_count: int, min_kmers: int, device: int, gfa: bool = False) -> dict:
    """pk_unitig_build on the staged table at `ptr`: the row arrays, the totals, the timings and `chunks`, an iterator over
    the FASTA bytes in slices of TEXT_SLICE; the builder, which holds the text in HBM, lives until the caller calls `close`.
    gfa: pk_unitig_graph behind the build: also the edge arrays, their totals and timings, and `gfa_chunks`, the GFA bytes
    in the same slices."""
    u = _lib.Unitigs(kmer_len, device=device)
    try:
        totals = u.build(ptr, min_count, max_count, min_kmers)
        _mark(f"{totals['n_nodes']} nodes, {totals['n_linear']} + {totals['n_circular']} unitigs")
        out = dict(totals, **u.rows(), **{key: val for key, val in u.timings().items() if key != "builds"})
        if gfa:
            graph = u.graph()
            _mark(f"{graph['n_edges']} edges")
            out.update(graph, **u.edges(), **u.graph_timings())
    except BaseException:
        u.close()
        raise

    def chunks(fetch, n_bytes):
        for off in range(0, n_bytes, TEXT_SLICE):
            yield memoryview(fetch(off, min(TEXT_SLICE, n_bytes - off)))
    out.update(chunks=chunks(u.text, totals["bytes"]), close=u.close)
    if gfa:
        out["gfa_chunks"] = chunks(u.gfa_text, out.pop("gfa_bytes"))
    return out


def build_unitigs(table, min_count: int = 1, max_count: int = 255, min_kmers: int = 1, device: int = 0, hbm_budget: int = None,
                  out_file=None, threads: int = DEFAULT_THREADS, stage=None, run=None, gfa: bool = False, gfa_file=None) -> dict:
    """The unitigs of `table`: a `.kin[.bgz]` path, a Header or a merger.ResidentTable.  Returns dict(first_addr, n_kmers,
    depth (U,) uint64, circular (U,) uint8, kmer_len, min_count, max_count, min_kmers, n_nodes, n_unitigs, n_circular,
    n_branching, n_short, nodes_short, bytes, bases, longest, n50, links_s, paths_s, cycles_s) and, without `out_file`, fasta
    (bytes); with it the FASTA is written there (through `.tmp` + rename) and `output` names it.  ValueError, with no file
    written, when no k-mer lies in the window.
    gfa: also the graph (README "Unitigs"): edge_from, edge_to (E,) uint64, edge_orient (E,) uint8 (bit 0: the from side is -,
    bit 1: the to side is -), n_edges, edges_dropped, n_dead_ends, edges_s, gfa_s and the GFA 1.0 text, as `gfa` (bytes) or,
    with `gfa_file`, written there with `gfa_output` naming it.  `run` is then called with gfa=True in addition and returns
    these keys and `gfa_chunks` too.  A `close` callable in what `run` returns is called when the texts are read, or on a failure.
    `stage(table, kmer_len, device, threads)` -> (ptr, free) and `run` (see run_build) default to stage_table and run_build
    (the CPU-only tests substitute both)."""
    table = as_headers([table], device)[0]
    kmer_len = validate([table], min_count, max_count, min_kmers)
    check_budget(table, kmer_len, device, hbm_budget)
    ptr, free = (stage or stage_table)(table, kmer_len, device, threads)
    _mark("table staged")
    try:
        got = (run or run_build)(ptr, kmer_len, min_count, max_count, int(min_kmers), device, **({"gfa": True} if gfa else {}))
    finally:
        free()                                               # the build is done with the table; the text is the builder's
    try:
        if got["n_nodes"] == 0:
            raise ValueError(f"{name_of(table)}: no k-mer has a count in the window {min_count}-{max_count}: no unitig to write")
        if out_file is None:
            fasta = b"".join(bytes(c) for c in got["chunks"])
        else:
            with atomic_write(out_file, "wb") as fhd:
                for c in got["chunks"]:
                    fhd.write(c)
        if gfa and gfa_file is None:
            gfa_text = b"".join(bytes(c) for c in got["gfa_chunks"])
        elif gfa:
            with atomic_write(gfa_file, "wb") as fhd:
                for c in got["gfa_chunks"]:
                    fhd.write(c)
    finally:
        for key in ("chunks", "gfa_chunks"):
            getattr(got.get(key), "close", lambda: None)()
        got.get("close", lambda: None)()                     # the builder and its texts in HBM go now, whatever was read or raised
    n_kmers = np.ascontiguousarray(got["n_kmers"], dtype=np.uint64)
    lengths = n_kmers + np.uint64(kmer_len - 1)
    result = {key: np.ascontiguousarray(got[key], dtype=np.uint64) for key in ("first_addr", "n_kmers", "depth")}
    result.update(circular=np.ascontiguousarray(got["circular"], dtype=np.uint8), kmer_len=kmer_len, min_count=int(min_count), max_count=int(max_count),
                  min_kmers=int(min_kmers), n_nodes=int(got["n_nodes"]), n_unitigs=int(n_kmers.size), n_circular=int(got["n_circular"]),
                  n_branching=int(got["n_branching"]), n_short=int(got["n_short"]), nodes_short=int(got["nodes_short"]), bytes=int(got["bytes"]),
                  bases=int(lengths.sum()), longest=int(lengths.max()) if lengths.size else 0, n50=n50(lengths),
                  **{key: float(got.get(key, 0.0)) for key in ("links_s", "paths_s", "cycles_s")})
    assert int(n_kmers.sum()) + result["nodes_short"] == result["n_nodes"], "the rows and the short unitigs do not hold every node once"
    assert result["n_unitigs"] == int(got["n_linear"]) + result["n_circular"] == int(result["circular"].size)
    if out_file is None:
        result["fasta"] = fasta
        assert len(fasta) == result["bytes"]
    else:
        result["output"] = str(out_file)
    if gfa:
        result.update(edge_from=np.ascontiguousarray(got["edge_from"], dtype=np.uint64), edge_to=np.ascontiguousarray(got["edge_to"], dtype=np.uint64),
                      edge_orient=np.ascontiguousarray(got["edge_orient"], dtype=np.uint8), n_edges=int(got["n_edges"]),
                      edges_dropped=int(got["edges_dropped"]), n_dead_ends=int(got["n_dead_ends"]),
                      **{key: float(got.get(key, 0.0)) for key in ("edges_s", "gfa_s")})
        assert result["n_edges"] == result["edge_from"].size == result["edge_to"].size == result["edge_orient"].size
        if gfa_file is None:
            result["gfa"] = gfa_text
        else:
            result["gfa_output"] = str(gfa_file)
    return result


def kmu_paths(project_name: str):
    return Path(f"{project_name}.unitigs.fa"), Path(f"{project_name}.kmu"), Path(f"{project_name}.kmu.json")


def gfa_path(project_name: str) -> Path:
    return Path(f"{project_name}.unitigs.gfa")


SCALARS = ("kmer_len", "min_count", "max_count", "min_kmers", "n_nodes")


def unitigs_records(project_name: str, indexes: List[Path], min_count: int = 1, max_count: int = 255, min_kmers: int = 1, device: int = 0,
                    threads: int = DEFAULT_THREADS, hbm_budget: int = None, stage=None, run=None, gfa: bool = False) -> dict:
    """The CLI's work: validate, build, write `<project>.unitigs.fa`, `<project>.kmu` and `<project>.kmu.json`; returns
    build_unitigs' result.  Every refusal (ValueError) comes before any file is written; no file is overwritten.
    gfa: also `<project>.unitigs.gfa`, the three edge arrays in the `.kmu` and their totals in the `.kmu.json`."""
    if len(indexes) != 1:
        raise ValueError(f"unitigs are built from exactly one table, got {len(indexes)}: {COMBINE}")
    check_window(min_count, max_count, min_kmers)
    out_file, kmu, meta = kmu_paths(project_name)
    gfa_file = gfa_path(project_name) if gfa else None
    refuse_files((out_file, kmu, meta) + ((gfa_file,) if gfa else ()), [])
    try:
        data = [table_entry(0, indexes[0], lambda kin: load_header(kin, device))]
        header = data[0]["header"]
        validate([header], min_count, max_count, min_kmers)
    except ValueError as exc:                                # an even kmer_len, or one above 17: there is no table to make of it
        raise ValueError(f"{exc} (unitigs take one table of an odd kmer_len <= 17; {COMBINE})" if "kmer_len" in str(exc) else str(exc)) from exc
    _mark("table verified")
    result = build_unitigs(header, min_count, max_count, min_kmers, device=device, hbm_budget=hbm_budget, out_file=out_file, threads=threads,
                           stage=stage, run=run, **({"gfa": True, "gfa_file": gfa_file} if gfa else {}))
    _mark(f"{out_file} written")
    lean_headers(data)
    output = {"project_name": project_name, "data": data, "output": result["output"]}
    output.update({key: int(result[key]) for key in SCALARS + ("n_unitigs", "n_circular", "n_branching", "n_short", "nodes_short", "bases", "longest", "n50")})
    output.update({key: result[key] for key in ("links_s", "paths_s", "cycles_s")})
    edges = {}
    if gfa:
        output.update(gfa=result["gfa_output"], **{key: result[key] for key in ("n_edges", "edges_dropped", "n_dead_ends", "edges_s", "gfa_s")})
        edges = {key: result[key] for key in ("edge_from", "edge_to", "edge_orient")}
    write_json(meta, output)
    with atomic_write(kmu, "wb") as fhd:
        np.savez_compressed(fhd, first_addr=result["first_addr"], n_kmers=result["n_kmers"], depth=result["depth"], circular=result["circular"], **edges,
                            **{key: np.int64(result[key]) for key in SCALARS})
    _mark("files renamed")
    return result


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Build the unitigs (the compacted de Bruijn graph) of one kmer database.")
    parser.add_argument("Project_Name", metavar="P", type=str, help="Project name (prefix of the output files)")
    parser.add_argument("Kmer_N", metavar="K", type=Path, nargs="+", help="One kin file (combine several with extract.py --table first)")
    parser.add_argument("--min-count", type=int, default=1, help="Minimum Kmer Count [1]")
    parser.add_argument("--max-count", type=int, default=255, help="Maximum Kmer Count [255]")
    parser.add_argument("--min-kmers", type=int, default=1, help="Unitigs of fewer k-mers are not written [1]")
    parser.add_argument("--gfa", action="store_true", help="Also write the unitig graph: <project>.unitigs.gfa (GFA 1.0), and its edges into the .kmu")
    parser.add_argument("--threads", type=int, default=DEFAULT_THREADS, help=f"Host threads reading / inflating the table [{DEFAULT_THREADS}]")
    return parser


def main(argv: List[str] = None) -> None:
    args = build_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    try:
        result = unitigs_records(args.Project_Name, args.Kmer_N, min_count=args.min_count, max_count=args.max_count, min_kmers=args.min_kmers,
                                 device=int(os.environ.get("PK_DEVICE", "0")), threads=args.threads, **({"gfa": True} if args.gfa else {}))
    except ValueError as exc:
        print(f"error: {exc}", file=sys.stderr)
        sys.exit(1)
    print(f"{result['n_unitigs']} unitigs ({result['n_circular']} circular) from {result['n_nodes']} k-mers, longest {result['longest']} bases, "
          f"N50 {result['n50']}, {result['output']}" + (f", {result['n_edges']} edges in {result['gfa_output']}" if args.gfa else ""))


if __name__ == "__main__":
    main()
