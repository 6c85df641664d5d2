#!/usr/bin/env python3
"""trim.py Project_Name reads.fq[.gz|.bgz] a.kin[.bgz] b.kin[.bgz] ... [--min-count A --max-count B] [--min-len L]
        [--mate reads_2.fq[.gz|.bgz]] [--rest] [--min-qual Q [--qual-offset 33|64]] [--threads T]

Cuts every read of a FASTQ file to the longest stretch that N k-mer tables cover (no counterpart in the reference): every
k-mer of the reads is looked up on the GPU as mask.py does, a base is covered when it lies in a window whose count lies in
the count window in at least one table, and a read keeps its longest run of covered bases -- line 2 and line 4 cut at the
same offsets, every other byte of the record as it is -- if the run is at least `--min-len` long (README "Trimming reads").
With `--min-qual` a base below the quality is an N and ends a run.  `<project>.trimmed.fq` (with `--mate` `trimmed_1.fq` and
`trimmed_2.fq`, a pair kept iff both mates are) holds the kept reads, uncompressed, `--rest` writes the others untrimmed;
`<project>.kmt` (np.savez_compressed: trim_start, trim_end, covered, seq_len, n_valid, keep and the parameters) and
`<project>.kmt.json` record the run.  FASTA input is refused (mask.py marks covered bases).  One device (PK_DEVICE).
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

from pykmer_amd.trim import main  # noqa: E402

if __name__ == "__main__":
    try:
        main()
    finally:
        _warm.join()           # an early exit (a refused argument) must not take the interpreter down under a HIP start-up in flight
