#!/usr/bin/env python3
"""query.py Project_Name queries.fa|.fq[.gz|.bgz] a.kin[.bgz] b.kin[.bgz] ... [--min-count --max-count --threads --bin W [--coords] --min-qual Q [--qual-offset 33|64]]

Per-record k-mer hits of a FASTA / FASTQ file against N k-mer tables (no counterpart in the reference): writes
`<project>.kmq` (np.savez_compressed: hits, depth (R,N) uint64; n_valid, seq_len (R,) uint64; kmer_len, min_count, max_count),
`<project>.kmq.json` (record names and the tables' metadata) and `<project>.kmq.tsv` (one line per record: the hits).  The
tables are staged in HBM (in groups if they do not fit: PK_MERGE_HBM_BUDGET) and every k-mer of the query is looked up on
the GPU; one device (PK_DEVICE).  `--bin W` also writes `<project>.kmb`, `.kmb.json` and `.kmb.tsv`: the same hits along each
record, one row per bin of W valid windows (README "Binned hits"); with `--coords` every row also carries its base
coordinates within the record (`bin_start`, `bin_end`; the tsv columns `start` and `end`).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _warm_device():
    """HIP start-up (~0.2 s) runs beside the imports and the argument / file set-up instead of after them."""
    try:
        from pykmer_amd import _rt         # ctypes only: starts before numpy is imported
        _rt.warm(int(os.environ.get("PK_DEVICE", "0")))
    except Exception:          # whatever is wrong is reported by the call that needs the device
        pass


if __name__ == "__main__":
    import threading
    _warm = threading.Thread(target=_warm_device, daemon=True)
    _warm.start()

from pykmer_amd.query import main  # noqa: E402

if __name__ == "__main__":
    try:
        main()
    finally:
        _warm.join()           # an early exit (a refused argument) must not take the interpreter down under a HIP start-up in flight
