"""Times the record selector (kmer_select.hip) on the read set of tools/query_bench.py -- 400 000 records of 1 kbp,
synth.generate(34, 400_000_000, 400_000) -- with the text in HBM (pk_select_feed_device), beside a plain device-to-device copy
of the same text, which is the yardstick of a streaming kernel, and beside the lookup of the same reads (phase 1 of filter.py).

The record offsets come from one parse of the text on the device (a counting indexer at k = 1, as filter.record_starts).  At
keep rates of 0 %, 50 % (random flags) and 100 %: one warm-up, then `--runs` timed passes, each a fresh selector fed the whole
text at once; `select_s` is the library's HIP-event time of the select kernels of the pass (pk_select_timings), `wall_s` the
host clock around the blocking call.  The kept bytes of the 50 % and 100 % passes are downloaded once and compared with numpy.
The copy: hipMemcpyDtoDAsync of the text between two HIP events on the null stream, the same number of runs, from the same
process.  The lookup: the reads against `--tables` tables at k = 15 (staged as tools/query_bench.py stages them), lookup_s and
the structure pass and squeeze from pk_indexer_timings.

    python tools/filter_bench.py [out.json] [--runs R] [--tables N] [--no-lookup]
    PK_QUERY_BENCH_BP / PK_QUERY_BENCH_TABLE_BP scale the read set and the table genomes down for a rehearsal.

Writes profiles/filter_select_reads.json (or out.json)."""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import synth  # noqa: E402
from pykmer_amd import _lib  # noqa: E402
from pykmer_amd.filter import starts_from  # noqa: E402


def hip_runtime():
    _lib.load()
    with open("/proc/self/maps") as fh:                      # the runtime the library brought in, not another one found by name
        paths = sorted({ln.split()[-1] for ln in fh if "libamdhip64" in ln})
    hip = ctypes.CDLL(paths[0])
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    return hip


def time_copy(hip, dst: int, src: int, n: int, runs: int):
    """Seconds of hipMemcpyDtoDAsync(dst, src, n) between two events on the null stream: one warm-up, then `runs`."""
    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc} while timing the copy")
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    ok(hip.hipEventCreate(ctypes.byref(a)))
    ok(hip.hipEventCreate(ctypes.byref(b)))
    out = []
    for i in range(runs + 1):
        ok(hip.hipEventRecord(a, None))
        ok(hip.hipMemcpyDtoDAsync(dst, src, n, None))
        ok(hip.hipEventRecord(b, None))
        ok(hip.hipEventSynchronize(b))
        ms = ctypes.c_float(0)
        ok(hip.hipEventElapsedTime(ctypes.byref(ms), a, b))
        if i:
            out.append(ms.value * 1e-3)
    return out


def main():
    argv, args, opts = sys.argv[1:], [], {"--runs": 5, "--tables": 13}
    while argv:
        a = argv.pop(0)
        if a in opts:
            opts[a] = int(argv.pop(0))
        elif not a.startswith("--"):
            args.append(a)
    runs, n_tables = opts["--runs"], opts["--tables"]
    genome_bp = int(os.environ.get("PK_QUERY_BENCH_BP", 800_000_000))
    table_bp = int(os.environ.get("PK_QUERY_BENCH_TABLE_BP", 40_000_000))
    if _lib.device_count() < 1:
        sys.exit("error: filter_bench.py needs a GPU")
    fa, bp = synth.generate(34, genome_bp // 2, max(1, genome_bp // 2000))
    fa = np.asarray(fa)
    n = int(fa.size)
    text, out = _lib.DeviceBuffer(n + 64), _lib.DeviceBuffer(n + 64)
    text.upload(fa)
    with _lib.Indexer(1) as ix:
        ix.feed_device(text.ptr, n)
        recs = ix.records(ix.finish()["n_records"])
    starts = starts_from(recs["name_off"], n)
    R = starts.size - 1
    lens = np.diff(starts).astype(np.int64)
    rng = np.random.default_rng(1)
    result = {"text_bytes": n, "bp": int(bp), "records": int(R), "runs": runs,
              "method": f"per keep rate 1 warm-up + {runs} passes of a fresh selector fed the whole text in HBM (pk_select_feed_device); select_s from HIP "
                        "events around the select kernels (pk_select_timings), wall_s around the blocking call; copy_s: hipMemcpyDtoDAsync of the same "
                        "text between two HIP events, same process",
              "rates": {}}
    for rate in (0, 50, 100):
        keep = np.zeros(R, dtype=np.uint8) if rate == 0 else np.ones(R, dtype=np.uint8) if rate == 100 else rng.integers(0, 2, R, dtype=np.uint8)
        selects, walls, kept = [], [], 0
        for i in range(runs + 1):
            with _lib.Selector(0) as sel:
                sel.set_records(starts, keep)
                t0 = time.perf_counter()
                kept = sel.feed_device(text.ptr, n, out.ptr, n)
                wall = time.perf_counter() - t0
                if i:
                    selects.append(sel.timings()["select_s"])
                    walls.append(wall)
                elif rate:                                   # once per rate: the bytes themselves
                    mask = np.repeat(keep != 0, lens)
                    want = fa[int(starts[0]):int(starts[-1])][mask]
                    assert kept == want.size and np.array_equal(out.download(kept), want), f"the kept bytes at {rate} % differ from numpy's"
                    del mask, want
        med = statistics.median(selects)
        result["rates"][str(rate)] = {"kept_bytes": int(kept), "kept_records": int(keep.sum()), "select_s_runs": selects, "select_s_median": med,
                                      "wall_s_median": statistics.median(walls),
                                      "text_GB_per_s": n / med / 1e9 if med > 0 else None,
                                      "kernels_run": bool(kept)}           # nothing kept: the host knows, and launches nothing
        print("keep", rate, json.dumps(result["rates"][str(rate)]), flush=True)
    copies = time_copy(hip_runtime(), out.ptr, text.ptr, n, runs)
    copy = statistics.median(copies)
    result.update(copy_s_runs=copies, copy_s_median=copy, copy_GB_per_s=n / copy / 1e9,
                  select_over_copy={r: v["select_s_median"] / copy for r, v in result["rates"].items()})
    print("copy", json.dumps(copies), flush=True)
    with _lib.Selector(0) as sel:                            # the host form once, for scale: the text up and the kept half down over PCIe
        sel.set_records(starts, rng.integers(0, 2, R, dtype=np.uint8))
        t0 = time.perf_counter()
        got = sel.feed(fa)
        result["host_feed_50"] = {"wall_s": time.perf_counter() - t0, "select_s": sel.timings()["select_s"], "kept_bytes": int(got.size)}
        del got
    out.free()
    if "--no-lookup" not in sys.argv:
        import query_bench
        query_bench.N = n_tables
        bufs = query_bench.stage_tables(table_bp)
        lookups, fronts = [], []
        with _lib.QueryIndexer(query_bench.K) as q:
            for i in range(runs + 1):
                q.reset()
                q.set_tables([b.ptr for b in bufs], 1, 255)
                q.feed_device(text.ptr, n)
                fin = q.finish()
                q.results(fin["n_records"])
                if i:
                    t = q.timings()
                    lookups.append(float(t["lookup_s"]))
                    fronts.append(float(t["scan_s"] + t["squeeze_s"]))
        for b in bufs:
            b.free()
        lookup = statistics.median(lookups)
        result["lookup"] = {"k": query_bench.K, "tables": n_tables, "lookup_s_runs": lookups, "lookup_s_median": lookup,
                            "structure_plus_squeeze_s_median": statistics.median(fronts),
                            "select_100_over_lookup": result["rates"]["100"]["select_s_median"] / lookup,
                            "select_50_over_lookup": result["rates"]["50"]["select_s_median"] / lookup}
    text.free()
    path = args[0] if args else os.path.join(ROOT, "profiles", "filter_select_reads.json")
    with open(path + ".tmp", "w") as fh:
        json.dump(result, fh, indent=1)
    os.replace(path + ".tmp", path)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
