"""What the CPU tests share: the stand-ins for the GPU (the oracle as indexer, host arrays as staged tables, the yardsticks as
the query's run hook) and the gloo launcher of the sharded merges.  Mechanisms only, no expectations."""
import os
import socket
import sys
import types

import numpy as np

import inputs
import oracle
import query_bins_ref
import query_coords_ref
import query_pairs_ref
import query_ref
import query_spectrum_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ files -------------------------
def write_kin(tmp_path, name, data, k, project=None):
    """<name>.<kk>.kin + .json as pykmer_amd.indexer writes them, with the oracle standing in for the GPU: a namespace of
    header, path (the .kin), result (the oracle's count) and table."""
    from pykmer_amd.header import Header
    fa = tmp_path / name
    fa.write_bytes(data)
    got = oracle.count_fasta(data, k)
    h = Header(project or str(fa), sample_name=name, input_file=str(fa), kmer_len=k)
    h._init_clean(overwrite=True)
    h.timer.update(got["total_bp"])
    h.num_kmers = got["num_kmers"]
    h.chromosomes = oracle.chromosomes(data, got["records"])
    got["table"].tofile(h.index_tmp_file)
    h.write_metadata_index_tmp_file(hist256=np.bincount(got["table"], minlength=256))
    os.rename(h.index_tmp_file, h.index_file_root)
    return types.SimpleNamespace(header=h, path=h.index_file_root, result=got, table=got["table"])


def family_indexes(tmp_path, manifest, n=13):
    """The first n inputs of the merger golden G7 (k = 7) as .kin files: their paths."""
    case = manifest["merger"]["G7_k7_n13_default"]
    return [write_kin(tmp_path, f"s{i:02d}.fa", inputs.make_input(spec), case["k"]).path for i, spec in enumerate(case["inputs"][:n])]


# ------------------------------------------------------------------ staging and device calls ------
def stage_host(group, device):
    """query's stage hook without a device: every Header's table read whole."""
    from pykmer_amd import query
    return query.Staged([g.read_table_slice(0, g.data_size) for g in group])


def stub_header(k, name, table=None):
    return types.SimpleNamespace(kmer_len=k, index_file=name, data_size=4 ** k, table=table)


def _add_rows(out, key, ref, rows, W):
    """The rows of an option as the run hook returns them: per record, and with bins also per bin."""
    if W is None:
        out[key] = rows[key]
    else:
        out["bin_" + key], out[key] = rows[key], ref.record_sums(rows[key], rows["bin_first"])


def query_hooks(text, dense, calls, k=5):
    """(tables, stage, run) for query_records without a device: `run` logs its keywords in `calls` and answers `text` from
    the yardstick of every option it is called with."""
    from pykmer_amd import query

    def stage(group, device=0, threads=None):
        return query.Staged([g.table for g in group])

    def run(query_file, kmer_len, ptrs, mn, mx, device, first, **kw):
        calls.append(dict(kw))
        W = kw.get("bin_windows")
        keys = ("seq_len", "n_valid", "hits", "depth")
        if W is None:
            want = query_ref.expected(text, kmer_len, ptrs, mn, mx)
        elif kw.get("coords"):
            want = query_coords_ref.expected(text, kmer_len, ptrs, mn, mx, W)
            keys += ("bin_hits", "bin_depth", "bin_first", "bin_start", "bin_end")
        else:
            want = query_bins_ref.expected(text, kmer_len, ptrs, mn, mx, W)
            keys += ("bin_hits", "bin_depth", "bin_first")
        out = {key: want[key] for key in keys}
        if kw.get("spectrum"):
            _add_rows(out, "spectrum", query_spectrum_ref, query_spectrum_ref.expected(text, kmer_len, ptrs, W), W)
        if kw.get("pairs"):
            _add_rows(out, "shared", query_pairs_ref, query_pairs_ref.expected(text, kmer_len, ptrs, mn, mx, W=W), W)
        if first:
            out["names"] = query_ref.names(text, want["records"])
        return out

    names = "abcdefghijklmnopqrs"
    tables = [types.SimpleNamespace(kmer_len=k, index_file=f"t{i}.kin", project_name=f"t{names[i]}", data_size=4 ** k, table=t,
                                    to_dict=lambda lean=True, i=i: {"kmer_len": k, "project_name": f"t{names[i]}"})
              for i, t in enumerate(dense)]
    return tables, stage, run


# ------------------------------------------------------------------ ranks over gloo ---------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _gloo_rank(rank, world, port, workdir, paths, part, save_matrix, merge_kw):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    from pykmer_amd import merger
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        seen = []

        def partial(headers, lo, hi, *a):
            out = part(headers, lo, hi, *a)                  # (windows,) device, threads pass through
            seen.append((lo, hi, sum(h.bytes_delivered for h in headers)))
            return out
        got = merger.merge(os.path.join(workdir, "dist"), paths, group=True, partial_fn=partial, **merge_kw)
        if save_matrix:
            np.save(os.path.join(workdir, f"matrix_rank{rank}.npy"), got[1])
        np.save(os.path.join(workdir, f"slice_rank{rank}.npy"), np.array(seen))
    finally:
        dist.destroy_process_group()


def gloo_merge(world, workdir, paths, part, save_matrix=False, **merge_kw):
    """merger.merge(<workdir>/dist, paths, group=True, **merge_kw) on `world` gloo ranks whose slice tallies come from the
    module-level function `part`.  Every rank leaves slice_rank<r>.npy, the (lo, hi, bytes delivered) of its passes, and
    with save_matrix matrix_rank<r>.npy."""
    import torch.multiprocessing as mp
    mp.spawn(_gloo_rank, args=(world, free_port(), str(workdir), paths, part, save_matrix, merge_kw), nprocs=world, join=True)
