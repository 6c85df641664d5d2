#!/usr/bin/env python3
"""mask.py Project_Name query.fa[.gz|.bgz] a.kin[.bgz] b.kin[.bgz] ... [--min-count A --max-count B] [--hard] [--invert]

Marks the bases of a FASTA file that N k-mer tables cover (no counterpart in the reference): every k-mer of the input is
looked up on the GPU as query.py does, a valid window matches when its count lies in the count window in at least one table,
and every base that lies in a matching window (with `--invert` every other valid base) is lower-cased, or with `--hard`
replaced by N, in a second pass over the input (README "Masking sequences").  `<project>.masked.fa` is the input's own bytes
at the same length, uncompressed; `<project>.kmm` (np.savez_compressed: masked, n_valid, seq_len and the parameters) and
`<project>.kmm.json` record the run.  FASTQ input is refused (filter.py selects reads).  One device (PK_DEVICE).
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

from pykmer_amd.mask import main  # noqa: E402

if __name__ == "__main__":
    try:
        main()
    finally:
        _warm.join()           # an early exit (a refused argument) must not take the interpreter down under a HIP start-up in flight
