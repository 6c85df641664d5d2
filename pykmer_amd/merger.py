"""Merger host side: N `.kin[.bgz]` tables in, `<project>.<min>-<max>.kma` + `.kma.json` out.

Same CLI, checks and outputs as the reference's merger.py (argparse :51-59, merge :80-210, main
:213-239).  The reference runs Header.calculate_distance once per pair in a process pool
(merger.py:137-153), reading both tables each time; here every table is staged in HBM once and ONE
kernel pass (pk_gram_device_partial) yields all N(N+1)/2 tallies.  With several GPUs the k-mer
address range is split across them; with torch.distributed initialised (one process per GPU) each
rank scans its slice and the N x N partials are summed by one all-reduce (RCCL over xGMI).  The CLI enters that
mode by itself under a launcher that sets WORLD_SIZE / RANK / LOCAL_RANK (torchrun), or with `--gpus N`, which
starts the N ranks before anything touches a GPU.
"""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from contextlib import closing
from pathlib import Path
from typing import List, Tuple

import numpy as np

from . import _lib
from .header import Header
from .output import _Encoder, atomic_write, write_json             # noqa: F401  (_Encoder: imported from here by older callers)
from .staging import ResidentTable, hbm_budget, piece_cuts, staged_pieces, sub_slices as _sub_slices   # noqa: F401
from .tables import EXTS, description_file, lean_headers, table_entry

DEFAULT_MIN_COUNT = Header.DEFAULT_MIN_COUNT
DEFAULT_MAX_COUNT = Header.DEFAULT_MAX_COUNT
DEFAULT_BUFFER_SIZE = Header.DEFAULT_BUFFER_SIZE
DEFAULT_BLOCK_SIZE = Header.DEFAULT_BLOCK_SIZE
DEFAULT_THREADS = 4


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Merge kmer databases.")
    parser.add_argument("Project_Name", metavar="P", type=str, help="Project name")
    parser.add_argument("Kmer_1", metavar="K", type=Path, nargs=1, help="List of kin files")
    parser.add_argument("Kmer_N", metavar="K", type=Path, nargs="+", help="List of kin files")
    parser.add_argument("--min-count", type=int, default=DEFAULT_MIN_COUNT, nargs="?", help=f"Minimum Kmer Count [{DEFAULT_MIN_COUNT}]")
    parser.add_argument("--max-count", type=int, default=DEFAULT_MAX_COUNT, nargs="?", help=f"Maximum Kmer Count [{DEFAULT_MAX_COUNT}]")
    parser.add_argument("--buffer-size", type=int, default=DEFAULT_BUFFER_SIZE, nargs="?", help=f"Buffer size [{DEFAULT_BUFFER_SIZE}]")
    parser.add_argument("--block-size", type=int, default=DEFAULT_BLOCK_SIZE, nargs="?", help=f"Block size [{DEFAULT_BLOCK_SIZE}]")
    parser.add_argument("--threads", type=int, default=DEFAULT_THREADS, nargs="?",
                        help=f"Host threads reading / inflating the tables [{DEFAULT_THREADS}]")
    parser.add_argument("--sweep", type=str, default=None,
                        help="several count windows in one run, e.g. 1-255,2-255,1-3 (tables staged once; one .kma each)")
    parser.add_argument("--spectrum", action="store_true",
                        help="one pass that tallies every pair's joint count spectrum: writes <P>.kms + .kms.json, from which every "
                             "requested window's .kma is derived (and any later one, without the .kin files: python -m pykmer_amd.spectrum)")
    parser.add_argument("--kwip", action="store_true",
                        help="kWIP's entropy-weighted kernel and distance instead of the pair tally: one pass writes <P>.kmo + "
                             ".kmo.json (the exact per-occupancy tallies), <P>.kern and <P>.dist, and no .kma (any weighting "
                             "again, without the .kin files: python -m pykmer_amd.kwip)")
    parser.add_argument("--patterns", action="store_true",
                        help="one pass per window that counts the k-mers of every presence pattern (which of the <= 16 tables hold "
                             "it): writes <P>.<min>-<max>.kmv + .kmv.json + .kmv.tsv (UpSet input) and the window's .kma, derived "
                             "from them (any subset's count again, without the .kin files: python -m pykmer_amd.patterns)")
    parser.add_argument("--gpus", type=int, default=0,
                        help="one process per GPU: the k-mer address range is split over N ranks and the N x N partials are "
                             "summed by one RCCL all-reduce (also entered under torchrun, which sets WORLD_SIZE / RANK)")
    return parser


def calculate_distance(k_index_file: str, l_index_file: str, min_count: int = DEFAULT_MIN_COUNT, max_count: int = DEFAULT_MAX_COUNT,
                       buffer_size: int = DEFAULT_BUFFER_SIZE, block_size: int = DEFAULT_BLOCK_SIZE) -> Tuple[int, int, int]:
    """merger.py:62-78: one pair, from paths."""
    k_header = Header(str(k_index_file), index_file=str(k_index_file), buffer_size=buffer_size)
    l_header = Header(str(l_index_file), index_file=str(l_index_file), buffer_size=buffer_size)
    return k_header.calculate_distance(l_header, min_count=min_count, max_count=max_count, block_size=block_size, threading=True)


def address_slice(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous slice of the k-mer address range owned by `rank` (multiples of 32 addresses)."""
    per = ((n + world - 1) // world + 31) & ~31
    lo = min(n, per * rank)
    return lo, min(n, lo + per)


def _flat_partial(headers: List[Header], lo: int, hi: int, device: int, threads: int, words: int, accumulate, staged_tables: int,
                  reserve: bool, acc_ptr: int = None, stats: dict = None):
    """The one accumulating loop of every merge pass.  Addresses [lo, hi) of every table are staged in HBM on `device`
    (staging.staged_pieces: sub-slice by sub-slice if they do not all fit; only bytes [lo, hi) of each file are read /
    inflated; ResidentTable entries are scanned where they lie) and `accumulate(ptrs, n, acc_ptr, device=)` runs once per
    staged piece, adding to a flat u64 accumulator of `words` words: at `acc_ptr` (zeroed by the caller -- the buffer an RCCL
    all-reduce then sums) or in a buffer of this call, which is then returned as one flat u64 host array.  `accumulate`
    returns its kernel seconds, which `stats["kernel_seconds"]` accumulates.

    `staged_tables` is how many table slices sub_slices fits into the HBM budget beside each other: N, or more when the
    pass keeps scratch per address of its own.  `reserve` keeps room in that budget for the accumulator this call allocates
    (41 MB of spectrum at N = 13, 4.2 GB at N = 128).  The pair tally passes False: its accumulator is a few KB and its cuts
    have never counted it; budgeting it would move the cuts, which is a change of behaviour of its own."""
    own_bytes = words * 8 if acc_ptr is None else 0
    cuts = piece_cuts(headers, lo, hi, staged_tables, device, reserve=own_bytes if reserve else 0)
    own = None
    if acc_ptr is None:
        own = _lib.DeviceBuffer(own_bytes, device)           # before the slice buffers, which the first piece allocates
    try:
        if own is not None:
            own.zero()
            acc_ptr = own.ptr
        with closing(staged_pieces(headers, cuts, device, threads)) as pieces:
            for ptrs, a, b in pieces:
                secs = accumulate(ptrs, b - a, acc_ptr, device=device)
                if stats is not None:
                    stats["kernel_seconds"] = stats.get("kernel_seconds", 0.0) + secs
        return None if own is None else own.download().view(np.uint64)
    finally:
        if own is not None:
            own.free()


def gpu_partial(headers: List[Header], lo: int, hi: int, windows, device: int, threads: int, acc_ptr: int = None, stats: dict = None):
    """The pair tally of addresses [lo, hi) for every (min_count, max_count) window: one kernel pass per group of windows
    over each staged piece (pk_gram_device_accumulate_windows; staging as _flat_partial).  W windows over N tables are a
    flat accumulator of W x N x N u64: at `acc_ptr` (zeroed by the caller) or in a buffer of this call, which is then
    returned as W host arrays of N x N."""
    N, W = len(headers), len(windows)

    def accumulate(ptrs, n, acc, device):
        return _lib.gram_device_accumulate_windows(ptrs, n, acc, windows, device=device)
    flat = _flat_partial(headers, lo, hi, device, threads, W * N * N, accumulate, N, False, acc_ptr=acc_ptr, stats=stats)
    return None if flat is None else list(flat.reshape(W, N, N))


def spectrum_partial(headers: List[Header], lo: int, hi: int, device: int, threads: int, acc_ptr: int = None, stats: dict = None):
    """One spectrum pass per staged piece of addresses [lo, hi) (pk_spectrum_device_accumulate; staging as _flat_partial).
    The tallies are accumulated in HBM: at `acc_ptr` (spectrum_words(N) u64, zeroed by the caller) or in a buffer of this
    call, which is then returned as one flat u64 host array: N x 256 histograms, then N(N-1)/2 x 255 x 255 joint bins."""
    return _flat_partial(headers, lo, hi, device, threads, _lib.spectrum_words(len(headers)), _lib.spectrum_device_accumulate,
                         len(headers), True, acc_ptr=acc_ptr, stats=stats)


def occgram_partial(headers: List[Header], lo: int, hi: int, device: int, threads: int, acc_ptr: int = None, stats: dict = None):
    """One occgram pass per staged piece of addresses [lo, hi) (pk_occgram_device_accumulate; staging as _flat_partial).
    The tallies are accumulated in HBM: at `acc_ptr` (occgram_words(N) u64, zeroed by the caller) or in a buffer of this
    call, which is then returned as one flat u64 host array: occ_hist (N+1), lin (N x N), gram (N x N(N+1)/2).  Beyond 16
    tables the pass keeps one occupancy byte per address in HBM: the sub-slices budget N + 1 tables."""
    N = len(headers)
    return _flat_partial(headers, lo, hi, device, threads, _lib.occgram_words(N), _lib.occgram_device_accumulate,
                         N + 1 if N > 16 else N, True, acc_ptr=acc_ptr, stats=stats)


def patterns_partial(headers: List[Header], lo: int, hi: int, windows, device: int, threads: int, acc_ptr: int = None, stats: dict = None):
    """One presence-pattern pass per window and staged piece of addresses [lo, hi) (pk_patterns_device_accumulate; staging
    as _flat_partial).  The tallies are accumulated in HBM: at `acc_ptr` (W x 2^N u64, zeroed by the caller) or in a buffer
    of this call, which is then returned as one flat u64 host array: window after window, 2^N bins each."""
    N = len(headers)
    words = _lib.patterns_words(N)

    def accumulate(ptrs, n, acc, device):
        return sum(_lib.patterns_device_accumulate(ptrs, n, acc + w * words * 8, mn, mx, device=device) for w, (mn, mx) in enumerate(windows))
    return _flat_partial(headers, lo, hi, device, threads, len(windows) * words, accumulate, N, True, acc_ptr=acc_ptr, stats=stats)


def _pair_flat(headers: List[Header], words: int, own_partial, threads: int, devices, group, partial_fn, stats) -> np.ndarray:
    """The one split-and-reduce of every merge pass: a flat accumulator of `words` u64 of all tables over the whole address
    range.  Single process: the range is split over `devices`, one host thread per device, and the partials are summed on
    the host.  With `group` (a torch.distributed process group, or True for the default group) this rank scans only its own
    slice on devices[0] and ONE all-reduce sums the ranks -- over RCCL ("nccl" on ROCm) on the accumulator where the kernel
    left it in HBM, through the host over gloo (rehearsals and CPU tests).  `partial_fn(headers, lo, hi, device, threads)`
    returns one slice's flat accumulator (default: `own_partial`, the only one that is handed `acc_ptr=` and `stats=`;
    the CPU-only tests substitute numpy)."""
    partial_fn = partial_fn or own_partial
    n = headers[0].data_size
    kw = {"stats": stats} if (stats is not None and partial_fn is own_partial) else {}
    if group is None:
        plan = [(d,) + address_slice(n, i, len(devices)) for i, d in enumerate(devices)]
        plan = [p for p in plan if p[2] > p[1]]
        with ThreadPoolExecutor(max_workers=max(1, len(plan))) as pool:
            parts = list(pool.map(lambda p: partial_fn(headers, p[1], p[2], p[0], max(1, threads // len(plan)), **kw), plan))
        total = np.zeros(words, dtype=np.uint64)
        for part in parts:
            total += part
        return total

    import torch
    import torch.distributed as dist
    pg = None if group is True else group
    dev = devices[0]
    lo, hi = address_slice(n, dist.get_rank(pg), dist.get_world_size(pg))
    on_gpu = dist.get_backend(pg) == "nccl"
    if partial_fn is own_partial and on_gpu:
        t = torch.zeros(words, dtype=torch.int64, device=torch.device("cuda", dev))
        torch.cuda.synchronize(dev)                             # zeroed before the passes (their own stream) add to it
        if hi > lo:
            own_partial(headers, lo, hi, dev, threads, acc_ptr=t.data_ptr(), stats=stats)
    else:
        total = np.zeros(words, dtype=np.uint64)
        if hi > lo:
            total += partial_fn(headers, lo, hi, dev, threads, **kw)
        t = torch.from_numpy(total.view(np.int64))
        if on_gpu:                                             # an RCCL group reduces device tensors only
            t = t.to(torch.device("cuda", dev))
    dist.all_reduce(t, group=pg)                               # over RCCL the accumulator has not left the device before the sum
    return t.cpu().numpy().view(np.uint64)


def pair_matrix(headers: List[Header], windows, threads: int = DEFAULT_THREADS, devices=(0,), group=None,
                partial_fn=None, stats: dict = None) -> List[np.ndarray]:
    """One N x N u64 per (min, max) window: [i][i] = valid addresses of table i, [i][j] (i<j) = addresses valid in both:
    the W x N x N words of all windows as one flat accumulator, split and reduced as _pair_flat does (so the partials of
    all windows are summed by ONE all-reduce).  `partial_fn(headers, lo, hi, windows, device, threads)` computes one slice's
    tallies as W arrays (default: gpu_partial, looked up when called; the CPU-only tests substitute the oracle)."""
    assert 1 <= len(headers) <= 128, "a pair tally takes 1 to 128 tables"
    N, W = len(headers), len(windows)

    def flat(pair_fn):
        def partial(headers, lo, hi, device, threads, **kw):
            parts = pair_fn(headers, lo, hi, windows, device, threads, **kw)
            return None if parts is None else np.asarray(parts, dtype=np.uint64).reshape(-1)
        return partial
    own = gpu_partial
    total = _pair_flat(headers, W * N * N, flat(own), threads, devices, group,
                       None if partial_fn in (None, own) else flat(partial_fn), stats)
    return list(total.reshape(W, N, N))


def pair_spectrum(headers: List[Header], threads: int = DEFAULT_THREADS, devices=(0,), group=None, partial_fn=None,
                  stats: dict = None) -> np.ndarray:
    """The spectrum accumulator of all tables over the whole address range (flat u64, spectrum_partial's layout), split
    as _pair_flat does; `partial_fn` defaults to spectrum_partial."""
    assert 2 <= len(headers) <= 128, "a spectrum takes 2 to 128 tables"
    return _pair_flat(headers, _lib.spectrum_words(len(headers)), spectrum_partial, threads, devices, group, partial_fn, stats)


def pair_occgram(headers: List[Header], threads: int = DEFAULT_THREADS, devices=(0,), group=None, partial_fn=None,
                 stats: dict = None) -> np.ndarray:
    """The occgram accumulator of all tables over the whole address range (flat u64, occgram_partial's layout), split
    as _pair_flat does; `partial_fn` defaults to occgram_partial."""
    assert 2 <= len(headers) <= 128, "kWIP takes 2 to 128 tables"
    return _pair_flat(headers, _lib.occgram_words(len(headers)), occgram_partial, threads, devices, group, partial_fn, stats)


def pair_patterns(headers: List[Header], windows, threads: int = DEFAULT_THREADS, devices=(0,), group=None, partial_fn=None,
                  stats: dict = None) -> np.ndarray:
    """The presence patterns of all tables over the whole address range, one row of 2^N u64 per (min, max) window, split
    and reduced as _pair_flat does (one all-reduce for all windows).  `partial_fn(headers, lo, hi, windows, device, threads)`
    computes one slice's flat W x 2^N tallies (default: patterns_partial; the CPU-only tests substitute numpy)."""
    from . import patterns as pat
    pat.check_tables(len(headers))
    N, W = len(headers), len(windows)

    def flat(fn):
        def partial(headers, lo, hi, device, threads, **kw):
            part = fn(headers, lo, hi, windows, device, threads, **kw)
            return None if part is None else np.asarray(part, dtype=np.uint64).reshape(-1)
        return partial
    own = flat(patterns_partial)
    total = _pair_flat(headers, W * _lib.patterns_words(N), own, threads, devices, group,
                       None if partial_fn in (None, patterns_partial) else flat(partial_fn), stats)
    return total.reshape(W, 1 << N)


def write_kma(project_name: str, mn: int, mx: int, data, matrix: np.ndarray) -> None:
    """`<project>.<min>-<max>.kma` (key `matrix`, merger.py:207) and its `.kma.json` (merger.py:189-201), each through
    `.tmp` + rename."""
    outfile = Path(f"{project_name}.{mn:03d}-{mx:03d}.kma")
    output = {"project_name": project_name, "min_count": mn, "max_count": mx, "data": data}
    write_json(Path(f"{outfile}.json"), output)
    with atomic_write(outfile, "wb") as fhd:
        np.savez_compressed(fhd, matrix=matrix)            # merger.py:207: key `matrix`


def print_matrix(matrix: np.ndarray) -> None:
    for k in range(matrix.shape[0] - 1):
        for l in range(k + 1, matrix.shape[0]):
            print(f"   matrix Total #{k:3d} {int(matrix[k, l, 0]):15,d} Total #{l:3d} {int(matrix[k, l, 1]):15,d} Shared {int(matrix[k, l, 2]):15,d}")


def merge(project_name: str, indexes: List[Path], min_count: int = DEFAULT_MIN_COUNT, max_count: int = DEFAULT_MAX_COUNT,
          buffer_size: int = DEFAULT_BUFFER_SIZE, block_size: int = DEFAULT_BLOCK_SIZE, threads: int = DEFAULT_THREADS,
          devices=(0,), group=None, partial_fn=None, windows=None, spectrum: bool = False, kwip: bool = False,
          patterns: bool = False):
    """merger.py:80-210.  `windows` (a list of (min_count, max_count)) turns the call into a sweep: the
    tables are staged once and one `.kma` + `.kma.json` is written per window (the reference re-runs
    the whole merge per threshold, README.md:57-61); the first window's matrix is returned.
    `spectrum` makes the one pass tally every pair's joint count spectrum instead (pair_spectrum; `partial_fn` then
    computes a slice's spectrum): `<project>.kms` + `.kms.json` are written, and every window's `.kma` is derived from
    the spectrum (pykmer_amd.spectrum), as any later window can be without the tables.
    `kwip` makes the one pass tally the occupancy-stratified Gram products instead (pair_occgram; `partial_fn` then computes
    a slice's accumulator): `<project>.kmo` + `.kmo.json`, `.kern` and `.dist` are written and no `.kma`; the call returns
    (data, kernel matrix).
    `patterns` makes one presence-pattern pass per window instead (pair_patterns; `partial_fn` then computes a slice's
    W x 2^N tallies): per window `<project>.<min>-<max>.kmv` + `.kmv.json` + `.kmv.tsv` are written, and the window's `.kma`
    is derived from the patterns (pykmer_amd.patterns).  At most 16 tables (ValueError otherwise, before any file is written)."""
    if patterns:
        from . import patterns as pat
        assert not spectrum and not kwip, "patterns takes no spectrum or kwip"
        pat.check_tables(len(indexes))
    if kwip:
        assert not spectrum and not windows and (min_count, max_count) == (DEFAULT_MIN_COUNT, DEFAULT_MAX_COUNT), \
            "kwip takes no count window, sweep or spectrum"
    windows = [(min_count, max_count)] if not windows else [tuple(w) for w in windows]
    for mn, mx in windows:
        assert mn >= 1
        assert mx <= 255
        assert not patterns or mn <= mx, f"an empty count window ({mn}-{mx}) has no patterns"
    assert buffer_size > 0
    assert block_size > 0
    assert len(indexes) > 0

    outfiles = [] if kwip else [Path(f"{project_name}.{mn:03d}-{mx:03d}.kma") for mn, mx in windows]
    assert not Path(project_name).exists(), f"project name ({project_name}) is a file. maybe forgot to pass project name as first argument?"
    for outfile in outfiles:
        assert not outfile.exists(), f"project output file ({outfile}) already exists. not overwriting."
    if spectrum:
        from . import spectrum as spec
        for f in spec.spectrum_paths(project_name):
            assert not f.exists(), f"spectrum output file ({f}) already exists. not overwriting."
    if patterns:
        for mn, mx in windows:
            for f in pat.pattern_paths(project_name, mn, mx):
                assert not f.exists(), f"pattern output file ({f}) already exists. not overwriting."
    if kwip:
        from . import kwip as kw
        for f in kw.kmo_paths(project_name):
            assert not f.exists(), f"kwip output file ({f}) already exists. not overwriting."

    indexes = [Path(p) for p in indexes]
    assert all(i.exists() for i in indexes)

    def load(kin):                                             # merger.py:108-117: the reference's checks, in its words
        kins = str(kin)
        assert kins.endswith(EXTS), f"all files must be .{Header.IND_EXT}[.bgz]: {kin}"
        desc = description_file(kin)
        assert desc.exists(), f"all .{Header.IND_EXT}[.{Header.COMP_EXT}] files must have a associated .{Header.IND_EXT}.{Header.DESC_EXT}: {desc}"
        return Header(kins, index_file=kins, buffer_size=buffer_size, device=devices[0])

    data, headers, kmer_len = [], [], None
    for pos, kin in enumerate(indexes):
        data.append(table_entry(pos, kin, load))
        header = data[-1]["header"]
        if kmer_len is None:
            kmer_len = header.kmer_len
        assert header.kmer_len == kmer_len, f"kmer_length differs. expected {kmer_len}, got {header.kmer_len}"
        headers.append(header)
    print()

    if kwip:
        total = pair_occgram(headers, threads=threads, devices=devices, group=group, partial_fn=partial_fn)
        occ_hist, lin, gram = kw.split_accumulator(total, len(headers))
        pairs = []
    elif spectrum:
        total = pair_spectrum(headers, threads=threads, devices=devices, group=group, partial_fn=partial_fn)
        hist, joint = spec.expand_accumulator(total, len(headers), headers[0].data_size)
        pairs = spec.window_pairs(hist, joint, windows)
    elif patterns:
        bins = pair_patterns(headers, windows, threads=threads, devices=devices, group=group, partial_fn=partial_fn)
        pairs = [pat.matrix_from_patterns(b, len(headers)) for b in bins]
    else:
        pairs = pair_matrix(headers, windows, threads=threads, devices=devices, group=group, partial_fn=partial_fn)
    lean_headers(data)
    is_writer = True
    if group is not None:
        import torch.distributed as dist
        is_writer = dist.get_rank(None if group is True else group) == 0
    if spectrum and is_writer:
        spec.save(project_name, hist, joint, kmer_len, headers[0].data_size, data)
    if kwip:
        ids = [v["header"]["input_file_name"] for v in data]
        kern = kw.kernel(lin, gram, kw.weights(len(headers)))
        dist = kw.distance(kern, ids)
        if is_writer:
            kw.save(project_name, occ_hist, lin, gram, kmer_len, headers[0].data_size, data)
            _, _, kern_path, dist_path = kw.kmo_paths(project_name)
            kw.write_matrix(kern_path, kern, ids)
            kw.write_matrix(dist_path, dist, ids)
        return data, kern

    matrices = []
    for w, ((mn, mx), outfile, pair) in enumerate(zip(windows, outfiles, pairs)):
        # (N,N,3): [k][l] = (total_k, total_l, shared) (merger.py:175-176); the diagonal, which the reference
        # never assigns in its uninitialised array (merger.py:136), is zero here
        matrix = _lib.gram_expand(pair)
        matrices.append(matrix)
        print_matrix(matrix)
        if not is_writer:
            continue
        if patterns:
            pat.save(project_name, mn, mx, bins[w], kmer_len, headers[0].data_size, data)
        write_kma(project_name, mn, mx, data, matrix)
    return data, matrices[0]


def parse_sweep(text: str):
    """`"1-255,2-255,1-3"` -> [(1, 255), (2, 255), (1, 3)]."""
    out = []
    for item in text.split(","):
        lo, hi = item.strip().split("-")
        out.append((int(lo), int(hi)))
    return out


def spawn_ranks(world: int, argv: List[str], script: str = None) -> int:
    """`merger.py ... --gpus N` without a launcher: start N ranks of this command line (one per GPU) and wait for them.
    The parent never touches a GPU (the root CLI skips its warm-up thread in this case), so the ranks are plain child
    processes of a process without a HIP context.  Rank 0 inherits stdout; the others print nothing."""
    import socket
    import subprocess
    import time
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    # the root CLI, whoever called main(): a rank must not start whatever sys.argv[0] happens to be (a test runner, say)
    script = script or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "merger.py")
    cmd = [sys.executable, script] + list(argv)
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen(cmd, env=env))
    killed = []
    while any(p.poll() is None for p in procs):
        if any(p.poll() not in (None, 0) for p in procs):       # a rank died: its peers would wait in the all-reduce for ever
            for p in procs:
                if p.poll() is None:
                    p.kill()                                     # exactly the children started above
                    killed.append(p)
            break
        time.sleep(0.05)
    codes = [p.wait() for p in procs]
    return max(abs(c) for p, c in zip(procs, codes) if p not in killed)   # the ranks' own statuses, not the -9 of those killed here


def _join_group():
    """One process per GPU: RANK / WORLD_SIZE / LOCAL_RANK / MASTER_* from the environment (torchrun, or spawn_ranks).
    Backend "nccl" (= RCCL over xGMI); PK_DIST_BACKEND=gloo rehearses the same path where ranks share a GPU.
    Returns (rank, device ordinal)."""
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    listed = [int(d) for d in os.environ.get("PK_DEVICES", "").split(",") if d != ""]
    n_dev = torch.cuda.device_count()
    device = listed[local % len(listed)] if listed else (local % n_dev if n_dev else 0)
    backend = os.environ.get("PK_DIST_BACKEND", "nccl")
    if backend == "nccl":
        torch.cuda.set_device(device)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", device))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, device


def main(argv: List[str] = None) -> None:
    """merger.py:213-239."""
    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_parser().parse_args(argv)
    indexes: List[Path] = args.Kmer_1 + args.Kmer_N
    if len(indexes) <= 1:
        print("needs at least 2 files")
        sys.exit(1)
    indexes.sort()                                             # matrix order = sorted path order (merger.py:228)
    windows = parse_sweep(args.sweep) if args.sweep else None
    if args.kwip and (args.spectrum or args.sweep or args.min_count != DEFAULT_MIN_COUNT or args.max_count != DEFAULT_MAX_COUNT):
        build_parser().error("--kwip takes no --spectrum, --sweep, --min-count or --max-count")
    if args.patterns and (args.spectrum or args.kwip):
        build_parser().error("--patterns takes no --spectrum or --kwip")
    if args.patterns:
        from . import patterns as pat
        try:
            pat.check_tables(len(indexes))
        except ValueError as e:
            print(f"error: {e}")
            sys.exit(1)
    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1:
            sys.exit(spawn_ranks(args.gpus, argv))
        devices = tuple(int(d) for d in os.environ.get("PK_DEVICES", "0").split(",") if d != "")
        merge(args.Project_Name, indexes, min_count=args.min_count, max_count=args.max_count, buffer_size=args.buffer_size,
              block_size=args.block_size, threads=args.threads, devices=devices or (0,), windows=windows, spectrum=args.spectrum,
              kwip=args.kwip, patterns=args.patterns)
        return
    # one rank of a multi-process merge: every rank validates and scans its address slice, rank 0 prints and writes
    import contextlib
    import torch.distributed as dist
    rank, device = _join_group()
    try:
        with contextlib.redirect_stdout(None) if rank else contextlib.nullcontext():
            merge(args.Project_Name, indexes, min_count=args.min_count, max_count=args.max_count, buffer_size=args.buffer_size,
                  block_size=args.block_size, threads=args.threads, devices=(device,), group=True, windows=windows,
                  spectrum=args.spectrum, kwip=args.kwip, patterns=args.patterns)
        dist.barrier()                                         # nobody leaves before rank 0 has renamed the outputs
    finally:
        dist.destroy_process_group()
