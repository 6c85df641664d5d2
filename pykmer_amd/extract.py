"""Extract host side: the k-mers that tell sample groups apart.  P "present" and A "absent" `.kin[.bgz]` tables in, the list
of k-mers behind the condition out.

With a count window min..max, `min_present` (default P) and `max_absent` (default 0), for every address x in [0, 4^k), the
canonical k-mer value exactly as a `.kin` is addressed:
    p(x) = #{ i present : min <= T_i[x] <= max }      (the validity test of the pair tally, tools.py:473-475)
    q(x) = #{ j absent  : T_j[x] >= 1 }               (an absent table holds x at any count; the window does not apply)
    x is selected iff p(x) >= min_present and q(x) <= max_absent
The result is the selected addresses in ascending order and, with each, the P raw bytes T_i[x] of the present tables,
inside the window or not.  P = 1 and A = 0 is a plain windowed dump of one table.  The reference has no such tool (its
README stops at the distance matrix); no table is written or changed.

The tables are staged in HBM slice by slice as the merger stages them (staging.staged_pieces); one streaming pass per piece
(pk_extract_device) compacts the selected addresses and their count rows in HBM, and pk_extract_text turns the addresses
into letters there.  One device (PK_DEVICE).

The same selection as a table (combine_tables, `--table OP`): one byte per address, 0 where x is not selected, else the
reduction OP over V(x) = { i present : min <= T_i[x] <= max } -- the bytes inside the window, not the raw rows --
    sum: min(255, sum of T_i[x])    min / max: the smallest / largest T_i[x]    count: |V(x)| = p(x)
written as a `.kin` + `.kin.json` that every tool reads (pk_extract_table_device, one streaming map per piece).  out[x] >= 1
exactly on the selected addresses.
"""
import argparse
import hashlib
import os
import sys
from pathlib import Path
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib, staging
from .indexer import _mark
from .header import Header
from .merger import DEFAULT_THREADS
from .output import atomic_write, write_json
from .query import load_header
from .tables import MAX_KMER_LEN, common_kmer_len, lean_headers, name_of as _name_of, table_entry   # noqa: F401

MAX_TABLES = 128                    # P + A: what one pk_extract_device call takes
PIECE_ALIGN = 2048                  # addresses: what the cuts of a piece are multiples of (and what always fits the output)
INITIAL_ROWS = 1 << 22              # output rows the first call has room for (fewer if the output budget holds fewer)
OUTPUT_SHARE = 8                    # the output arrays get 1 / OUTPUT_SHARE of the HBM budget, the staged slices the rest
OPS = _lib.TABLE_OPS                # ("sum", "min", "max", "count"): what combine_tables / --table reduce the present bytes with
HIST_BYTES = 256 * 8                # the value histogram of a combined table, kept in HBM across the pieces


def _kmer_len_of(table) -> int:
    k = getattr(table, "kmer_len", None)
    if k is not None:
        return int(k)
    size, k = int(table.data_size), 0                        # a merger.ResidentTable knows only its 4^k
    while 4 ** k < size:
        k += 1
    if 4 ** k != size:
        raise ValueError(f"{_name_of(table)}: a table of {size} bytes is no 4^k")
    return k


def _file_of(table):
    f = getattr(table, "index_file", None)
    return os.path.abspath(str(f)) if f else None


def kmx_paths(project_name: str) -> Tuple[Path, Path, Path]:
    return Path(f"{project_name}.kmx"), Path(f"{project_name}.kmx.json"), Path(f"{project_name}.kmx.txt")


def _refuse_existing(files) -> None:
    for f in files:
        if Path(f).exists():
            raise ValueError(f"project output file ({f}) already exists. not overwriting.")


def validate(present: Sequence, absent: Sequence, min_count: int = 1, max_count: int = 255, min_present: int = None, max_absent: int = 0,
             project_name: str = None) -> Tuple[int, int]:
    """The checks that need no device; returns (kmer_len, min_present with its default filled in).  `present` / `absent`:
    Headers, merger.ResidentTables or anything with kmer_len (or data_size).  `project_name`: also refuse to overwrite its
    output files."""
    P, A = len(present), len(absent)
    if not 1 <= min_count <= max_count <= 255:
        raise ValueError(f"the count window must satisfy 1 <= min <= max <= 255, got {min_count}-{max_count}")
    if P < 1:
        raise ValueError("an extraction needs at least one present table")
    if P + A > MAX_TABLES:
        raise ValueError(f"an extraction takes at most {MAX_TABLES} tables, got {P} present + {A} absent")
    min_present = P if min_present is None else int(min_present)
    if not 1 <= min_present <= P:
        raise ValueError(f"min_present must lie in 1..{P} (the present tables), got {min_present}")
    if not 0 <= int(max_absent) <= A:
        raise ValueError(f"max_absent must lie in 0..{A} (the absent tables), got {max_absent}")
    tables = list(present) + list(absent)
    kmer_len = common_kmer_len(tables, "extract", _kmer_len_of)
    files = [f for f in map(_file_of, tables) if f]
    for f in files:
        if files.count(f) > 1:
            raise ValueError(f"{f} is named twice: a table is present or absent, and listed once")
    if project_name is not None:
        _refuse_existing(kmx_paths(project_name))
    return kmer_len, min_present


class DeviceCall:
    """pk_extract_device on one address range of a staged piece, with output arrays in HBM that grow to the capacity asked
    for.  call(ptrs, off, n, first_addr, cap) -> (n_selected, None) when more than `cap` addresses are selected, else
    (n_selected, (addr, counts, text or None)) downloaded.  extract_kmers' `call=` substitutes anything of this shape."""

    def __init__(self, n_present: int, kmer_len: int, min_count: int, max_count: int, min_present: int, max_absent: int, device: int = 0,
                 text: bool = False):
        self.P, self.k, self.device, self.text = n_present, kmer_len, device, text
        self.params = (min_count, max_count, min_present, max_absent)
        self.cap, self.bufs, self.kernel_seconds = 0, [], 0.0

    def free(self):
        for b in self.bufs:
            b.free()
        self.cap, self.bufs = 0, []

    def _reserve(self, cap: int):
        if cap <= self.cap:
            return
        self.free()                                          # first: the old and the new arrays need not fit beside each other
        sizes = [cap * 8, cap * self.P] + ([cap * (self.k + 1)] if self.text else [])
        self.bufs = [_lib.DeviceBuffer((s + 15) & ~15, self.device) for s in sizes]
        self.cap = cap

    def __call__(self, ptrs, off: int, n: int, first_addr: int, cap: int):
        self._reserve(max(1, cap))
        count, fits, secs = _lib.extract_device([p + off for p in ptrs], self.P, n, first_addr, *self.params, dev_addr_out=self.bufs[0].ptr,
                                                dev_counts_out=self.bufs[1].ptr, cap=max(1, cap), device=self.device)
        self.kernel_seconds += secs
        if not fits:
            return count, None
        _mark(f"addresses {first_addr}..{first_addr + n - 1}: {count} selected")
        if count == 0:
            return 0, (np.zeros(0, dtype=np.uint64), np.zeros((0, self.P), dtype=np.uint8), np.zeros((0, self.k + 1), dtype=np.uint8) if self.text else None)
        text = None
        if self.text:
            _lib.extract_text(self.bufs[0].ptr, count, self.k, self.bufs[2].ptr, device=self.device)
            text = self.bufs[2].download(count * (self.k + 1)).reshape(count, self.k + 1)
        addr = self.bufs[0].download(count * 8).view(np.uint64)
        counts = self.bufs[1].download(count * self.P).reshape(count, self.P)
        _mark(f"{count} rows downloaded")
        return count, (addr, counts, text)


def _extract_range(call, ptrs, off: int, n: int, first_addr: int, state: dict, parts: list) -> None:
    """Addresses [first_addr, first_addr + n), which lie `off` bytes into the staged piece: call with the current capacity;
    grow it to the reported count if the output budget holds that many rows, else halve the range (cuts at multiples of
    PIECE_ALIGN; pointer offset and first address advance together) and take the halves in ascending order."""
    state["calls"] += 1
    count, res = call(ptrs, off, n, first_addr, state["cap"])
    if res is None and (count <= state["max_rows"] or n <= PIECE_ALIGN):
        state["cap"] = count                                 # PIECE_ALIGN addresses always fit: max_rows >= PIECE_ALIGN
        state["calls"] += 1
        count, res = call(ptrs, off, n, first_addr, state["cap"])
        assert res is not None, "the selection changed between two calls on the same slices"
    if res is None:
        half = (n // 2 + PIECE_ALIGN - 1) // PIECE_ALIGN * PIECE_ALIGN
        _extract_range(call, ptrs, off, half, first_addr, state, parts)
        _extract_range(call, ptrs, off + half, n - half, first_addr + half, state, parts)
        return
    parts.append(res)


def stage_pieces(tables: Sequence, lo: int, hi: int, device: int, threads: int, reserve: int, budget: int):
    """The staged pieces (ptrs, a, b) of [lo, hi), in ascending order: N slices beside each other in `budget` bytes less the
    `reserve` of the output arrays (staging.piece_cuts), staged by staging.staged_pieces."""
    return staging.staged_pieces(tables, staging.piece_cuts(tables, lo, hi, len(tables), device, reserve, budget), device, threads)


def extract_kmers(present: Sequence, absent: Sequence = (), min_count: int = 1, max_count: int = 255, min_present: int = None,
                  max_absent: int = 0, device: int = 0, hbm_budget: int = None, threads: int = DEFAULT_THREADS, text: bool = False,
                  initial_rows: int = INITIAL_ROWS, stage=None, call=None) -> dict:
    """The selected k-mers of `present` / `absent`: Headers, merger.ResidentTables or `.kin[.bgz]` paths.  Returns dict(addr
    (M,) uint64 ascending, counts (M, P) uint8 -- column i is present table i --, text (M, k + 1) uint8 lines of k letters +
    newline if `text`, kmer_len, min_count, max_count, min_present, max_absent, n_present, n_absent, n_selected, ...).

    `hbm_budget` (bytes; default PK_MERGE_HBM_BUDGET, else 80 % of the free HBM) holds the staged slices and the output
    arrays: 1 / OUTPUT_SHARE of it is the output's (never less than PIECE_ALIGN rows), the slices are cut to fit the rest.
    A piece that selects more rows than the output holds is taken in halves.
    `stage(tables, lo, hi, device, threads, reserve, budget)` -> iterable of (ptrs, a, b) and `call` (see DeviceCall)
    default to stage_pieces and a DeviceCall (the CPU-only tests substitute both)."""
    present = [load_header(t, device) if isinstance(t, (str, os.PathLike)) else t for t in present]
    absent = [load_header(t, device) if isinstance(t, (str, os.PathLike)) else t for t in absent]
    kmer_len, min_present = validate(present, absent, min_count, max_count, min_present, max_absent)
    tables, P = present + absent, len(present)
    row_bytes = 8 + P + (kmer_len + 1 if text else 0)
    budget = staging.hbm_budget(device, hbm_budget)
    out_budget = max(PIECE_ALIGN * row_bytes, budget // OUTPUT_SHARE)
    state = {"max_rows": out_budget // row_bytes, "calls": 0}
    state["cap"] = max(1, min(state["max_rows"], int(initial_rows)))
    own = None
    if call is None:
        call = own = DeviceCall(P, kmer_len, min_count, max_count, min_present, int(max_absent), device=device, text=text)
    pieces = (stage or stage_pieces)(tables, 0, 4 ** kmer_len, device, threads, out_budget, budget)
    parts, n_pieces = [], 0
    try:
        for ptrs, a, b in pieces:
            _mark(f"addresses {a}..{b - 1} staged")
            n_pieces += 1
            _extract_range(call, ptrs, 0, b - a, a, state, parts)
    finally:
        getattr(pieces, "close", lambda: None)()             # a generator frees its slice buffers now, not when it is collected
        if own is not None:
            own.free()
    addr = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, dtype=np.uint64)
    counts = np.concatenate([p[1] for p in parts]) if parts else np.zeros((0, P), dtype=np.uint8)
    result = {"addr": np.ascontiguousarray(addr, dtype=np.uint64), "counts": np.ascontiguousarray(counts, dtype=np.uint8).reshape(-1, P),
              "kmer_len": kmer_len, "min_count": int(min_count), "max_count": int(max_count), "min_present": min_present,
              "max_absent": int(max_absent), "n_present": P, "n_absent": len(absent), "n_selected": int(addr.size), "n_pieces": n_pieces,
              "n_calls": state["calls"], "kernel_seconds": own.kernel_seconds if own is not None else 0.0}
    if text:
        lines = np.concatenate([p[2] for p in parts]) if parts else np.zeros((0, kmer_len + 1), dtype=np.uint8)
        result["text"] = np.ascontiguousarray(lines, dtype=np.uint8).reshape(-1, kmer_len + 1)
    return result


class TableCall:
    """pk_extract_table_device on one staged piece, with the piece's output slice and the table's value histogram in HBM.
    call(ptrs, a, b, out) fills out[a:b] (downloaded straight into it); call.hist256() is the histogram of everything
    written so far, zeros included.  combine_tables' `call=` substitutes anything of this shape."""

    def __init__(self, n_present: int, op: str, min_count: int, max_count: int, min_present: int, max_absent: int, device: int = 0):
        self.P, self.op, self.device = n_present, op, device
        self.params = (min_count, max_count, min_present, max_absent)
        self.slice, self.hist, self.addresses, self.kernel_seconds = None, None, 0, 0.0

    def free(self):
        for b in (self.slice, self.hist):
            if b is not None:
                b.free()
        self.slice = self.hist = None

    def __call__(self, ptrs, a: int, b: int, out: np.ndarray) -> None:
        n = b - a
        if self.hist is None:
            self.hist = _lib.DeviceBuffer(HIST_BYTES, self.device)
            self.hist.zero()
        if self.slice is None or self.slice.n < n:
            if self.slice is not None:
                self.slice.free()                            # first: the old and the new slice need not fit beside each other
            self.slice = _lib.DeviceBuffer((n + 15) & ~15, self.device)
        self.kernel_seconds += _lib.extract_table_device(ptrs, self.P, n, *self.params, self.op, self.slice.ptr, self.hist.ptr, device=self.device)
        self.slice.download_into(out[a:b])
        self.addresses += n
        _mark(f"addresses {a}..{b - 1}: table bytes downloaded")

    def hist256(self) -> np.ndarray:
        hist = np.zeros(256, dtype=np.uint64) if self.hist is None else self.hist.download().view(np.uint64).copy()
        hist[0] = self.addresses - int(hist[1:].sum())       # the device tallies the values 1 .. 255
        return hist


def stage_table_pieces(tables: Sequence, lo: int, hi: int, device: int, threads: int, reserve: int, budget: int):
    """stage_pieces with room for one more slice beside the N staged ones: the output's."""
    return staging.staged_pieces(tables, staging.piece_cuts(tables, lo, hi, len(tables) + 1, device, reserve, budget), device, threads)


def combine_tables(present: Sequence, absent: Sequence = (), op: str = "sum", min_count: int = 1, max_count: int = 255, min_present: int = None,
                   max_absent: int = 0, out: np.ndarray = None, device: int = 0, hbm_budget: int = None, threads: int = DEFAULT_THREADS,
                   stage=None, call=None) -> dict:
    """The selection of `present` / `absent` (as extract_kmers takes them) as a table of 4^k bytes: 0 where an address is
    not selected, else `op` (one of OPS) over the present bytes inside the window.  Returns dict(table -- `out`, a writable
    uint8 array or memmap of 4^k bytes, or a fresh array --, hist256 (256,) uint64, n_selected (its non-zero bytes), op,
    kmer_len, min_count, max_count, min_present, max_absent, n_present, n_absent, n_pieces, kernel_seconds).

    The pieces are cut so that the P + A slices and one output slice fit `hbm_budget` (as extract_kmers reads it) beside
    each other; every piece is one device call and one download into out[a:b], and the histogram stays in HBM until the
    last.  `stage(tables, lo, hi, device, threads, reserve, budget)` and `call` (see TableCall) default to
    stage_table_pieces and a TableCall."""
    if op not in OPS:
        raise ValueError(f"unknown table operation {op!r}: expected one of {', '.join(OPS)}")
    present = [load_header(t, device) if isinstance(t, (str, os.PathLike)) else t for t in present]
    absent = [load_header(t, device) if isinstance(t, (str, os.PathLike)) else t for t in absent]
    kmer_len, min_present = validate(present, absent, min_count, max_count, min_present, max_absent)
    size = 4 ** kmer_len
    if out is None:
        out = np.empty(size, dtype=np.uint8)
    if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == (size,) and out.flags.c_contiguous and out.flags.writeable):
        raise ValueError(f"out must be a writable contiguous uint8 array of 4^{kmer_len} = {size} bytes")
    tables, P = present + absent, len(present)
    own = None
    if call is None:
        call = own = TableCall(P, op, min_count, max_count, min_present, int(max_absent), device=device)
    pieces = (stage or stage_table_pieces)(tables, 0, size, device, threads, HIST_BYTES, hbm_budget)
    n_pieces = 0
    try:
        for ptrs, a, b in pieces:
            _mark(f"addresses {a}..{b - 1} staged")
            n_pieces += 1
            call(ptrs, a, b, out)
        hist = np.ascontiguousarray(call.hist256(), dtype=np.uint64)
    finally:
        getattr(pieces, "close", lambda: None)()             # a generator frees its slice buffers now, not when it is collected
        if own is not None:
            own.free()
    assert hist.shape == (256,) and int(hist.sum()) == size, "the histogram does not cover the table"
    return {"table": out, "hist256": hist, "n_selected": size - int(hist[0]), "op": op, "kmer_len": kmer_len, "min_count": int(min_count),
            "max_count": int(max_count), "min_present": min_present, "max_absent": int(max_absent), "n_present": P, "n_absent": len(absent),
            "n_pieces": n_pieces, "kernel_seconds": own.kernel_seconds if own is not None else 0.0}


SCALARS = ("kmer_len", "min_count", "max_count", "min_present", "max_absent", "n_present", "n_absent")


def write_kmx_json(project_name: str, result: dict, data: list, **more) -> None:
    """`<project>.kmx.json`: the scalars, n_selected, the tables' metadata (present tables first) and whatever `more` holds."""
    assert len(data) == int(result["n_present"]) + int(result["n_absent"])
    output = {"project_name": project_name, "n_selected": int(result["n_selected"]), "data": data, **more}
    output.update({key: int(result[key]) for key in SCALARS})
    write_json(kmx_paths(project_name)[1], output)


def write_kmx(project_name: str, result: dict, data: list) -> None:
    """`<project>.kmx` (np.savez_compressed: addr, counts and the scalars), `.kmx.json` (the scalars, n_selected and the
    tables' metadata, present tables first: the order of the columns of counts) and, when the result holds the text,
    `.kmx.txt` (one k-mer per line, in addr order); each through `.tmp` + rename."""
    kmx, meta, txt = kmx_paths(project_name)
    addr = np.ascontiguousarray(result["addr"], dtype=np.uint64)
    counts = np.ascontiguousarray(result["counts"], dtype=np.uint8)
    assert counts.shape == (addr.size, int(result["n_present"]))
    write_kmx_json(project_name, dict(result, n_selected=addr.size), data)
    if result.get("text") is not None:
        lines = np.ascontiguousarray(result["text"], dtype=np.uint8)
        assert lines.shape == (addr.size, int(result["kmer_len"]) + 1)
        with atomic_write(txt, "wb") as fhd:
            lines.tofile(fhd)
    with atomic_write(kmx, "wb") as fhd:
        np.savez_compressed(fhd, addr=addr, counts=counts, **{key: np.int64(result[key]) for key in SCALARS})


def table_paths(project_name: str, kmer_len: int) -> Tuple[Path, Path, Path]:
    """What `--table` writes: `<project>.<KK>.kin`, its `.kin.json` and `<project>.kmx.json`."""
    kin = f"{project_name}.{kmer_len:02d}.{Header.IND_EXT}"
    return Path(kin), Path(f"{kin}.{Header.DESC_EXT}"), kmx_paths(project_name)[1]


def write_table(project_name: str, op: str, data: list, device: int, **combine) -> dict:
    """combine_tables straight into `<project>.<KK>.kin.tmp`, renamed once it is complete, then its `.kin.json`
    (Header.write_derived_metadata_file) and `<project>.kmx.json`.  `data`: the table entries, Headers still in them.  An
    empty selection is an error (a `.kin.json` asserts a non-zero num_kmers); no file is left behind when the pass fails."""
    headers = [v["header"] for v in data]
    n_present = sum(v["role"] == "present" for v in data)
    kmer_len = int(headers[0].kmer_len)
    kin = table_paths(project_name, kmer_len)[0]
    _refuse_existing(table_paths(project_name, kmer_len) + (Path(f"{kin}.{Header.COMP_EXT}"),))   # a .kin.bgz would be read in the .kin's place
    header = Header(os.path.basename(project_name), input_file=project_name, kmer_len=kmer_len, device=device)
    tmp = Path(f"{kin}.{Header.TMP}")
    print(f"saving {kin}")
    table = None
    try:
        table = np.memmap(tmp, dtype=np.uint8, mode="w+", shape=(4 ** kmer_len,))
        result = combine_tables(headers[:n_present], headers[n_present:], op=op, out=table, device=device, **combine)
        if result["n_selected"] == 0:
            raise ValueError(f"no k-mer is selected (count window {result['min_count']}-{result['max_count']}, min_present {result['min_present']} "
                             f"of {result['n_present']}, max_absent {result['max_absent']} of {result['n_absent']}): no table is written")
        table.flush()
        sha = hashlib.sha256()
        for at in range(0, table.size, 1 << 24):
            sha.update(table[at:at + (1 << 24)])
        del result["table"]                                  # the mapping goes before the file is renamed
        table = None
        tmp.rename(kin)
    except BaseException:
        table = None
        tmp.unlink(missing_ok=True)
        raise
    _mark("table written")
    sources = [(f"{v['role']}:{v['header'].project_name}", v["header"].num_kmers) for v in data]
    header.write_derived_metadata_file(str(kin), result["hist256"], sources, checksum=sha.hexdigest())
    lean_headers(data)
    write_kmx_json(project_name, result, data, table=op, table_file=kin)
    result["table_file"] = str(kin)
    return result


def extract(project_name: str, present: List[Path], absent: List[Path] = (), min_count: int = 1, max_count: int = 255, min_present: int = None,
            max_absent: int = 0, kmers: bool = False, device: int = 0, threads: int = DEFAULT_THREADS, hbm_budget: int = None, table: str = None) -> dict:
    """The CLI's work: validate, extract, write the files; returns extract_kmers' result -- or, with `table` (one of OPS),
    write_table's: the selection as `<project>.<KK>.kin` instead of the `.kmx` list."""
    if table is not None and table not in OPS:
        raise ValueError(f"unknown table operation {table!r}: expected one of {', '.join(OPS)}")
    if table is not None and kmers:
        raise ValueError("--table writes a table and no k-mer list: it cannot be combined with --kmers")
    _refuse_existing(kmx_paths(project_name)[1:2] if table else kmx_paths(project_name))
    data = []
    for role, kins in (("present", present), ("absent", absent)):
        for kin in kins:
            data.append(table_entry(len(data), kin, lambda kin: load_header(kin, device), role=role))
    headers, n_present = [v["header"] for v in data], len(list(present))
    validate(headers[:n_present], headers[n_present:], min_count, max_count, min_present, max_absent, project_name=None if table else project_name)
    _mark("tables verified")
    if table is not None:
        result = write_table(project_name, table, data, device, min_count=min_count, max_count=max_count, min_present=min_present,
                             max_absent=max_absent, hbm_budget=hbm_budget, threads=threads)
        _mark("files renamed")
        return result
    result = extract_kmers(headers[:n_present], headers[n_present:], min_count, max_count, min_present, max_absent, device=device,
                           hbm_budget=hbm_budget, threads=threads, text=kmers)
    lean_headers(data)
    write_kmx(project_name, result, data)
    _mark("files renamed")
    return result


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Extract the k-mers present in some kmer databases and absent from others.")
    parser.add_argument("Project_Name", metavar="P", type=str, help="Project name (prefix of the output files)")
    parser.add_argument("--present", metavar="K", type=Path, nargs="+", required=True, help="kin files that must hold the k-mer (in the count window)")
    parser.add_argument("--absent", metavar="K", type=Path, nargs="*", default=[], help="kin files that must not hold it (at any count)")
    parser.add_argument("--min-count", type=int, default=1, help="Minimum Kmer Count in a present table [1]")
    parser.add_argument("--max-count", type=int, default=255, help="Maximum Kmer Count in a present table [255]")
    parser.add_argument("--min-present", type=int, default=None, help="present tables that must hold the k-mer [all of them]")
    parser.add_argument("--max-absent", type=int, default=0, help="absent tables that may hold it all the same [0]")
    parser.add_argument("--kmers", action="store_true", help="also write <P>.kmx.txt: the k-mers as letters, one per line")
    parser.add_argument("--table", choices=OPS, default=None,
                        help="write the selection as a table, <P>.<KK>.kin + .kin.json, instead of the .kmx list: per selected k-mer the sum "
                             "(saturating at 255), min or max of the present counts inside the window, or the number of such tables")
    parser.add_argument("--threads", type=int, default=DEFAULT_THREADS, help=f"Host threads reading / inflating the tables [{DEFAULT_THREADS}]")
    return parser


def main(argv: List[str] = None) -> None:
    args = build_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    try:
        result = extract(args.Project_Name, args.present, args.absent, min_count=args.min_count, max_count=args.max_count,
                         min_present=args.min_present, max_absent=args.max_absent, kmers=args.kmers,
                         device=int(os.environ.get("PK_DEVICE", "0")), threads=args.threads, table=args.table)
    except ValueError as exc:
        print(f"error: {exc}", file=sys.stderr)
        sys.exit(1)
    print(f"{result['n_selected']:,d} k-mers selected, {result['n_present']} present + {result['n_absent']} absent tables, "
          f"{result['n_pieces']} staged piece(s)" + (f", table {result['table_file']} ({result['op']})" if args.table else ""))


if __name__ == "__main__":
    main()
