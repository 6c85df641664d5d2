#!/usr/bin/env python3
"""correct.py Project_Name reads.fq[.gz|.bgz] a.kin[.bgz] b.kin[.bgz] ... [--min-count A --max-count B] [--min-windows M]
        [--min-qual Q [--qual-offset 33|64]] [--threads T]

Puts single wrong base calls of the reads of a FASTQ file back from N k-mer tables (no counterpart in the reference): every
k-mer of the reads is looked up on the GPU as trim.py does; a valid base that no matching window covers, in a run of at least
kmer_len valid bases, is a candidate, and it is corrected when exactly one other base makes every window that holds it match
(README "Correcting reads").  Every candidate is judged against the uncorrected read; a candidate with fewer than
`--min-windows` windows (the ends of a read) is left alone.  With `--min-qual` a base below the quality is an N: never
corrected, the end of a run.  `<project>.corrected.fq` is the input with the corrected bytes replaced, case kept, nothing
else changed, uncompressed; `<project>.kme` (np.savez_compressed: candidates, untried, corrected, ambiguous, seq_len, n_valid,
the list of fixes and the parameters) and `<project>.kme.json` record the run.  FASTA input is refused.  All tables are
staged together.  One device (PK_DEVICE).
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

from pykmer_amd.correct import main  # noqa: E402

if __name__ == "__main__":
    try:
        main()
    finally:
        _warm.join()           # an early exit (a refused argument) must not take the interpreter down under a HIP start-up in flight
