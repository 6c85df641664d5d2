#!/usr/bin/env python3
"""filter.py Project_Name queries.fa|.fq[.gz|.bgz] a.kin[.bgz] b.kin[.bgz] ... [--min-count A --max-count B] [--min-hits H] [--min-percent P]
          [--min-tables M] [--invert] [--rest] [--mate reads_2.fq[.gz|.bgz]] [--pair-rule any|both] [--min-qual Q [--qual-offset 33|64]]

Writes the records of a FASTA / FASTQ file that match N k-mer tables (no counterpart in the reference): every k-mer of the
input is looked up on the GPU as query.py does, a table matches a record with at least H hits on at least P percent of its
valid windows, a record matches when at least M tables do, and the matching records (with `--invert` the others) are written
to `<project>.kept.fa|.fq` as the input's own bytes, selected on the GPU in a second pass over the input (README "Filtering
sequences").  `--rest` also writes the other records, `--mate` treats two files as pairs (`kept_1`, `kept_2`, ...).
`<project>.kmf` (np.savez_compressed: keep, match, hits, n_valid, seq_len and the parameters) and `<project>.kmf.json` record
the decision.  One device (PK_DEVICE).
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

from pykmer_amd.filter import main  # noqa: E402

if __name__ == "__main__":
    try:
        main()
    finally:
        _warm.join()           # an early exit (a refused argument) must not take the interpreter down under a HIP start-up in flight
