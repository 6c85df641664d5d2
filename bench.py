#!/usr/bin/env python3
"""bench.py -- headline benchmark: bp/s of canonical k-mer counting at k=15 on the ~800 Mbp synthetic
genome (BASELINE.json configs[1]), one genome per GPU (weak scaling), plus the
N=13 k=15 merge scan as a secondary figure.

A step = one whole indexing job on HBM-resident input: reset, structure pass (line / record state of every 64-byte
piece, bases classified once), squeeze (packed 2-bit stream), bucket layout from a sample, fused k-mer assembly +
level-1 sort (k_walk_sort), level-2 sort, bucket count into the 4^k table (which also keeps the value histogram),
side list.  Prints ONE JSON line on rank 0.  The merge legs call pykmer_amd.merger.pair_matrix, the function
merger.py runs.

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line: the headline, the stage
split of the timed steps and the roofline derived from them.  --full adds what takes runs of its own: the merge legs
(N=13 and N=32, with the threshold sweep), the CPU baselines with their parity checks against the GPU, and the
end-to-end timings of the two CLIs; --no-merge / --no-merge32 / --no-cpu / --no-e2e leave pieces of it out.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--bp 800000000] [--dump-outputs DIR]
                    [--full [--no-merge] [--no-merge32] [--no-cpu] [--no-e2e]]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: 8.0 TB/s spec


def spawn_ranks(world: int) -> int:
    """`python bench.py --gpus N` without a launcher: start N ranks of this script (one per GPU) and relay
    rank 0's JSON line.  The parent never touches the GPU (no torch import, no HIP call), so nothing here is
    an exec of a GPU-initialised process; the ranks are plain child processes."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    import threading
    chunks = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    while any(p.poll() is None for p in procs):
        if any(p.poll() not in (None, 0) for p in procs):       # a rank died: its peers would wait in a collective for ever
            for p in procs:
                if p.poll() is None:
                    p.kill()                                     # exactly the children started above
            break
        time.sleep(0.2)
    rcs = [p.wait() for p in procs]
    reader.join(timeout=10)
    sys.stdout.write(b"".join(c for c in chunks if c).decode())
    sys.stdout.flush()
    return max(abs(rc) for rc in rcs)


def end_to_end(fasta, total_bp, k, device):
    import shutil
    import subprocess
    import tempfile
    import synth
    from pykmer_amd import _lib
    res = {}
    table = np.empty(4 ** k, dtype=np.uint8)
    _lib.count_fasta(fasta, k, device=device, table_out=table)            # first call: allocations, page faults of `table`
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        _lib.count_fasta(fasta, k, device=device, table_out=table)
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    _lib.load().pk_count_release()
    res["indexer_host_buffers"] = {"t_e2e_s": best, "bp_per_s": total_bp / best,
                                   "what": "pk_count_fasta on pageable host buffers, best of 3 after one warm call: H2D of the text, the count, D2H of the 4^k table"}
    del table
    tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        def run(*argv):
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable] + list(argv), capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-500:])
            return time.perf_counter() - t0
        big = os.path.join(tmp, "genome.fa")
        fasta.tofile(big)
        t = run(os.path.join(ROOT, "indexer.py"), big, "genome", str(k))
        res["indexer_cli"] = {"t_e2e_s": t, "bp_per_s": total_bp / t,
                              "what": f"`indexer.py genome.fa genome {k}` as a fresh process, files on tmpfs: process start -> .kin + .kin.json renamed"}
        os.remove(big)
        kins = []
        for i in range(13):
            g, _ = synth.family(i, 20_000_000)
            p = os.path.join(tmp, f"s{i:02d}.fa")
            g.tofile(p)
            run(os.path.join(ROOT, "indexer.py"), p, f"s{i}", str(k))
            kins.append(f"{p}.{k:02d}.kin")
        t = run(os.path.join(ROOT, "merger.py"), os.path.join(tmp, "proj"), *kins, "--threads", "8")
        res["merger_cli"] = {"t_e2e_s": t, "n_tables": 13,
                             "what": f"`merger.py proj 13 x .{k:02d}.kin` (raw 4^{k}-byte tables on tmpfs) as a fresh process: process start -> .kma + .kma.json renamed"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return res


def save_output(out_dir, name, a, dtype=np.float64):
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, name + ".npy"), np.asarray(a, dtype=dtype))


def dump_indexer_outputs(out_dir, ix, fin):
    """What a caller of the timed path gets back from its last step: Indexer.finish()'s numbers, the records and the
    4^k table.  The table (1 GiB at k=15) is sampled: 1024 stretches of 4096 entries at seeded offsets, the same on every
    run, or the whole table when it is smaller than that; its values go out as float32, everything else as float64
    (exact for these integer counts)."""
    save_output(out_dir, "num_kmers", [fin["num_kmers"]])
    save_output(out_dir, "total_bp", [fin["total_bp"]])
    save_output(out_dir, "hist256", fin["hist256"])
    recs = ix.records(fin["n_records"])
    for f in recs.dtype.names:
        save_output(out_dir, "records_" + f, recs[f])
    n, stretch, n_stretches = ix.table_bytes, 4096, 1024
    if n <= stretch * n_stretches:
        starts, stretch = np.zeros(1, dtype=np.int64), n
    else:
        starts = np.sort(np.random.default_rng(0).choice(n // stretch, size=n_stretches, replace=False)) * stretch
    sample = np.empty((len(starts), stretch), dtype=np.uint8)
    for row, start in zip(sample, starts):
        ix.table_slice_to_host(row, int(start))
    save_output(out_dir, "table_sample", sample, np.float32)
    save_output(out_dir, "table_sample_offsets", starts)


def cpu_info():
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {"model": model, "nproc": os.cpu_count(), "usable_by_this_process": len(os.sched_getaffinity(0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5,
                    help="untimed steps first: the GPU needs a few (about 20 ms of work) to reach its clocks -- with one warm-up step the same "
                         "build measures 3.77-3.79 ms per step, with five or more 3.69-3.70")
    ap.add_argument("--bp", type=int, default=800_000_000, help="genome size (default: config 2)")
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--merge-n", type=int, default=13)
    ap.add_argument("--merge-bp", type=int, default=40_000_000, help="genome size behind each merge table")
    ap.add_argument("--full", action="store_true",
                    help="after the bench line's steps, also run the merge legs, the CPU baselines and the end-to-end CLI timings")
    ap.add_argument("--no-merge", action="store_true", help="skip the merge legs (and the merge matrices of --dump-outputs)")
    ap.add_argument("--no-merge32", action="store_true", help="skip the 32-table merge (config 5 shape)")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-e2e", action="store_true", help="with --full: skip the end-to-end (disk -> files) timings of the two CLIs")
    ap.add_argument("--cpu-bp", type=int, default=160_000_000, help="sample size for the CPU baseline")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="threads of the all-cores CPU legs (default 0 = every core this process may run on)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one computed (and the merge matrices) as DIR/<name>.npy "
                         "(rank 0; inputs are seeded, so two builds can be compared output for output)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    # the bench measures the library as shipped: no alternate build, no kernel switches (experiments: tools/)
    switches = [v for v in ("PK_LIB", "PK_K15", "PK_K6_BYTES", "PK_GRAM_MW", "PK_DENSE_SHIFT", "PK_WG1", "PK_GRID2", "PK_XCD", "PK_SPARSE_MAX")
                if v in os.environ]
    # (kernel experiments, tools/bench_variants.sh: PK_EXPERIMENT=1 lets them through and the JSON line says so)
    assert not switches or os.environ.get("PK_EXPERIMENT") == "1", f"experiment switches set in the environment: {switches}"

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))

    import torch
    import synth
    from pykmer_amd import _lib

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    n_dev = torch.cuda.device_count()
    if local >= n_dev:                    # rehearsal of the multi-rank path on a box with fewer GPUs than ranks
        local = local % max(n_dev, 1)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local)
        backend = os.environ.get("PK_DIST_BACKEND", "nccl")       # nccl = RCCL on ROCm; gloo only for rehearsals
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()

    # ---- input: one synthetic genome per rank, resident in HBM before the clock starts
    k = args.k
    fasta, total_bp = synth.c2(args.bp, seed=2 + rank)
    n_bytes = int(fasta.size)
    d_fasta = torch.empty(n_bytes + 64, dtype=torch.uint8, device=dev)
    d_fasta[:n_bytes].copy_(torch.from_numpy(fasta))
    torch.cuda.synchronize()

    ix = _lib.Indexer(k, device=local)

    def step():
        ix.reset()
        ix.feed_device(d_fasta.data_ptr(), n_bytes)
        return ix.finish()

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    acc = {"scan_s": 0.0, "squeeze_s": 0.0, "walk_sort_s": 0.0, "partition_s": 0.0, "bucket_s": 0.0, "finalize_s": 0.0, "zero_s": 0.0}
    relayouts = recounted = 0
    fin = None
    for _ in range(args.steps):
        fin = step()
        t = ix.timings()
        for key in acc:
            acc[key] += t[key]
        relayouts += t["relayouts"]
        recounted = t["buckets_recounted"]
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
        bp_all = torch.tensor([total_bp], dtype=torch.int64, device=dev)
        dist.all_reduce(bp_all)
        bp_job = int(bp_all.item())
    else:
        bp_job = total_bp
    assert fin["total_bp"] == total_bp, (fin["total_bp"], total_bp)
    if args.dump_outputs and rank == 0:                                 # before the merge section re-uses the indexer
        dump_indexer_outputs(args.dump_outputs, ix, fin)
    value = bp_job * args.steps / elapsed
    avg = {key: v / args.steps for key, v in acc.items()}

    # ---- roofline of the dominant kernel: k_walk_sort (packed bases -> canonical k-mers -> level-1 runs), or
    # k_bucket_count where writing the table dominates (k=17).  Algorithmic bytes = FASTA read once + table written
    # once (F + 4^k, 2.36 B/bp on C2 at k=15); duration = that kernel's launches timed with HIP events on
    # the indexer's own stream (pk_indexer_timings).
    alg_bytes = n_bytes + 4 ** k
    dominant, dom_avg = "k_walk_sort", avg["walk_sort_s"]
    if avg["bucket_s"] > dom_avg:
        dominant, dom_avg = "k_bucket_count", avg["bucket_s"]
    achieved = alg_bytes / dom_avg / 1e9
    # measured HBM bytes per launch come from rocprofv3 PMC passes (FETCH_SIZE / WRITE_SIZE cannot be read from inside the
    # process): tools/hbm_traffic.py turns the two CSVs into profiles/hbm_traffic.json, collected on exactly this workload
    traffic = pipeline_traffic = traffic_source = None
    tname = "hbm_traffic.json" if k == 15 else f"hbm_traffic_k{k}.json"
    tp = os.path.join(ROOT, "profiles", tname)
    if os.path.exists(tp) and k in (15, 17) and args.bp == 800_000_000:
        with open(tp) as fh:
            tj = json.load(fh)
        if dominant in tj:
            traffic = tj[dominant].get("bytes_per_launch")
            pipeline_traffic = tj.get("_pipeline_bytes_per_step")
            traffic_source = f"profiles/{tname} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this workload, not measured in this run)"
    out = {
        "metric": f"bp/s k-mer counted (k={k}, {world} GPU{'s' if world > 1 else ''})",
        "value": value, "unit": "bp/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "config": {"workload": f"k={k} canonical k-mer count of one {total_bp / 1e6:.0f} Mbp synthetic genome per GPU "
                               f"(SURVEY 8d C2, seed 2+rank), 4^{k} table resident in HBM",
                   "fasta_bytes": n_bytes, "num_kmers": fin["num_kmers"], "parallelism": f"{world} independent genome(s)"},
        "roofline": {"bound": "hbm", "kernel": dominant, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                     "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": dom_avg * 1e3,
                     "pipeline_traffic_bytes_per_step": pipeline_traffic,
                     "pipeline_hbm_GBps": (pipeline_traffic / (elapsed / args.steps) / 1e9) if pipeline_traffic else None},
        "stage_ms": {"reset": avg["zero_s"] * 1e3, "structure_scans": avg["scan_s"] * 1e3, "squeeze": avg["squeeze_s"] * 1e3,
                     "walk_sort_kernel": avg["walk_sort_s"] * 1e3,
                     "bucket_layout_and_level2": (avg["partition_s"] - avg["walk_sort_s"]) * 1e3,
                     "bucket_count": avg["bucket_s"] * 1e3, "finish": avg["finalize_s"] * 1e3,
                     "bucket_relayouts": relayouts, "buckets_recounted_per_step": recounted},
        "t_kernel_s": elapsed / args.steps,
    }
    if switches:
        out["experiment_switches"] = {v: os.environ[v] for v in switches}

    # ---- secondary: N x N merge scan over N tables resident in HBM, address range sharded over ranks
    # (N=13: BASELINE configs[2]; N=32: configs[4], the LDS-tiled kernel).  Not part of `value`.
    def merge_section(N):
        # the product path: pykmer_amd.merger.pair_matrix on tables that stayed in HBM (ResidentTable) -- the same function
        # merger.py calls; with several ranks it scans this rank's address slice into an accumulator in HBM and sums the
        # N x N partials with one all-reduce over RCCL (merger.py:137-178's pool, replaced)
        from pykmer_amd import merger
        n = 4 ** k
        lo, hi = merger.address_slice(n, rank, world)
        slices = []
        for i in range(N):
            fa, _ = synth.family(i, args.merge_bp)
            ix.reset()
            ix.feed(fa)
            ix.finish()
            sl = torch.empty(hi - lo, dtype=torch.uint8, device=dev)
            ix.table_slice_to_device(sl.data_ptr(), lo, hi - lo)   # this rank's address slice stays in HBM
            slices.append(sl)
        tabs = [merger.ResidentTable(sl.data_ptr(), hi - lo, n, device=local, first=lo) for sl in slices]
        ptrs = [s.data_ptr() for s in slices]
        group = True if dist is not None else None

        def timed(windows, reps=8):
            # the first launches over tables this kernel has not touched yet are slow (3.9, 2.3, 3.3 ms, then 2.25-2.29 for
            # as long as one cares to repeat: `tools/gram_stagger.py`): one untimed call, the best of the seven behind it
            best, kern, pairs = None, None, None
            for rep in range(reps):
                barrier()
                t0 = time.perf_counter()
                stats = {}
                pairs = merger.pair_matrix(tabs, windows, devices=(local,), group=group, stats=stats)
                barrier()
                dt = time.perf_counter() - t0
                if rep and (best is None or dt < best):
                    best, kern = dt, stats.get("kernel_seconds")
            if dist is not None:                                   # slowest rank defines the merge time
                tt = torch.tensor([best], dtype=torch.float64, device=dev)
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                best = float(tt.item())
            return best, kern, pairs
        if args.full:
            best, kern, pairs = timed([(1, 255)])
        else:                                                      # --dump-outputs alone: the matrix from one untimed call
            pairs = merger.pair_matrix(tabs, [(1, 255)], devices=(local,), group=group)
        total = pairs[0].astype(np.int64)
        if args.dump_outputs and rank == 0:
            save_output(args.dump_outputs, f"merge_n{N}_pairs", pairs[0])
        assert all(total[i, j] <= min(total[i, i], total[j, j]) for i in range(N) for j in range(i + 1, N))
        if not args.full:
            return None
        res = {"n_tables": N, "k": k, "seconds": best, "kernel_seconds_rank0": kern, "algorithmic_bytes": N * n,
               "kernel_GBps_aggregate": N * n / kern / 1e9 if world == 1 else None,
               "end_to_end_GBps_aggregate": N * n / best / 1e9,
               "sharding": f"address range / {world} + all_reduce(N*N u64)" if world > 1 else "single GPU",
               "path": "pykmer_amd.merger.pair_matrix (ResidentTable inputs)"}
        # threshold sweep (README.md:57-61: the reference re-merges per threshold): eight windows from one pass over the tables
        sweep = [(1, 255), (2, 255), (3, 255), (4, 255), (5, 255), (8, 255), (1, 50), (2, 20)]
        s_best, s_kern, s_pairs = timed(sweep, reps=3)
        assert np.array_equal(s_pairs[0].astype(np.int64), total)
        res["sweep8_seconds"] = s_best
        res["sweep8_kernel_seconds_rank0"] = s_kern
        res["sweep8_over_one_scan"] = (s_kern / kern) if (kern and s_kern) else None
        if rank == 0 and world == 1 and not args.no_cpu:
            # CPU baseline of the merge: the reference's pair loop (tools.py:439-493 per pair, merger.py:137-153 over a
            # pool) restated in C, on a bounded slice of the address range of the SAME tables; the pair loop's cost is
            # linear in the slice, so the full-size figure is the slice time scaled by n / slice
            import oracle
            pairs = N * (N - 1) // 2
            m = max(2048, min(n, int(2.5e9 / (2 * pairs))) & ~2047)
            host = [sl[:m].cpu().numpy() for sl in slices]
            t0 = time.perf_counter()
            ref = oracle.gram_mt(host, 1, 255, 1)
            dt1 = time.perf_counter() - t0
            avail = len(os.sched_getaffinity(0))
            threads = max(1, min(args.cpu_threads, avail) if args.cpu_threads > 0 else avail)
            t0 = time.perf_counter()
            ref_mt = oracle.gram_mt(host, 1, 255, threads)
            dtn = time.perf_counter() - t0
            gpu_slice, _ = _lib.gram_device_partial(ptrs, m, 1, 255, device=local)
            same = bool(np.array_equal(_lib.gram_expand(gpu_slice), ref) and np.array_equal(ref, ref_mt))
            res["cpu_baseline"] = {
                "value": dt1 * n / m, "unit": "s", "cores": 1, "kind": "port",
                "sample": f"oracle pko_gram_mt, {pairs} pairs over addresses [0, {m}) of the same {N} tables ({dt1:.1f} s), scaled by {n // m}",
                "all_cores": {"value": dtn * n / m, "unit": "s", "cores": threads, "kind": "port",
                              "sample": f"same slice, pairs spread over {threads} threads ({dtn:.2f} s)"},
                "slice_equals_gpu": same, "host": cpu_info()}
        return res

    if not args.no_merge and (args.full or args.dump_outputs):           # secondary objects: never allowed to cost the bench line
        def guarded(n_tables):
            # every rank must take the same path (the sharded merge all-reduces), so errors are not swallowed
            # when running distributed; nor when the section only writes outputs, which must not go missing quietly
            if dist is not None or not args.full:
                return merge_section(n_tables)
            try:
                return merge_section(n_tables)
            except Exception as exc:
                return {"n_tables": n_tables, "error": f"{type(exc).__name__}: {exc}"}
        legs = [("merge", args.merge_n)] + ([("merge_n32", 32)] if args.merge_n != 32 and not args.no_merge32 else [])
        for key, n_tables in legs:
            res = guarded(n_tables)
            if res is not None:
                out[key] = res

    # ---- CPU baseline: the oracle's C restatement, one core, bounded sample of the same workload
    if args.full and rank == 0 and world == 1 and not args.no_cpu:
        try:
            import oracle
            fa, bp = synth.c2(args.cpu_bp, seed=2)
            tab = np.zeros(4 ** k, dtype=np.uint8)
            t0 = time.perf_counter()
            r = oracle.count_fasta(fa, k, table=tab)
            dt = time.perf_counter() - t0
            out["cpu_baseline"] = {"value": bp / dt, "unit": "bp/s", "cores": 1, "kind": "port",
                                   "sample": f"oracle/kmer_oracle.c on a {bp / 1e6:.0f} Mbp C2-profile genome at k={k} ({dt:.1f} s)",
                                   "host_cores_available": os.cpu_count()}
            # the same port on the host cores this process may use, on the WHOLE workload; its table is also
            # compared with the one the GPU built -- a second, independent full-size parity check
            avail = len(os.sched_getaffinity(0))
            threads = max(1, min(args.cpu_threads, avail) if args.cpu_threads > 0 else avail)
            out["cpu_baseline"]["host"] = cpu_info()
            step()                                                          # the merge section reused the indexer: recount
            gpu_table = ix.table_to_host()
            t0 = time.perf_counter()
            mt = oracle.count_fasta_mt(fasta, k, threads)
            dt_mt = time.perf_counter() - t0
            if mt is not None:
                same = bool(mt["num_kmers"] == fin["num_kmers"] and mt["total_bp"] == total_bp and np.array_equal(mt["table"], gpu_table))
                out["cpu_baseline"]["all_cores"] = {"value": total_bp / dt_mt, "unit": "bp/s", "cores": threads, "kind": "port",
                                                    "sample": f"oracle/kmer_oracle_mt.c on the whole {total_bp / 1e6:.0f} Mbp workload at k={k} ({dt_mt:.1f} s)",
                                                    "table_equals_gpu_table": same}
                if not same:                                                # reported, not fatal: the bench line must still be printed
                    print("WARNING: all-cores CPU port and GPU table disagree", file=sys.stderr)
            del gpu_table, mt
            # the like-for-like anchor for the reference's 0.5 Mbp/s: its O(k)-per-window Python algorithm, restated
            from oracle import pyoracle
            small, sbp = synth.c2(300_000, seed=2)
            recs = list(pyoracle.records(small.tobytes().decode()))
            t0 = time.perf_counter()
            n_win = sum(1 for _, seq, _ in recs for _ in pyoracle.windows(seq, k))
            out["cpu_baseline"]["python_restatement_bp_per_s"] = sbp / (time.perf_counter() - t0)
            out["cpu_baseline"]["python_restatement_sample"] = f"oracle/pyoracle.py windows() on {sbp} bp ({n_win} k-mers), 1 core"
        except Exception as exc:                                        # the bench line is printed regardless
            out.setdefault("cpu_baseline", {})["error"] = f"{type(exc).__name__}: {exc}"
    # ---- end to end (t_e2e beside t_kernel).  (1) the one-shot C-ABI call on host buffers: PCIe both ways
    # (0.81 GB up, 1 GiB table down) inside the call; (2) the two CLIs as fresh processes on tmpfs files: process start ->
    # .kin/.kin.json (.kma/.kma.json) renamed, i.e. interpreter + HIP start-up, disk, PCIe, both sha256 sums.
    if args.full and rank == 0 and world == 1 and not args.no_e2e:
        try:
            out["e2e"] = end_to_end(fasta, total_bp, k, local)
        except Exception as exc:
            out["e2e"] = {"error": f"{type(exc).__name__}: {exc}"}
    if rank == 0:
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
