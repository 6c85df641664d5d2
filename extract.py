#!/usr/bin/env python3
"""extract.py Project_Name --present a.kin[.bgz] ... [--absent c.kin[.bgz] ...] [--min-count --max-count --min-present --max-absent --kmers --threads]

The k-mers that tell sample groups apart (no counterpart in the reference): every canonical k-mer that at least --min-present
(default: all) of the present tables hold with a count in --min-count..--max-count and at most --max-absent (default 0) of
the absent tables hold at any count.  Writes `<project>.kmx` (np.savez_compressed: addr (M,) uint64 ascending, counts (M,P)
uint8 = the present tables' counts of each k-mer, and the parameters), `<project>.kmx.json` (the parameters, n_selected and
the tables' metadata with their role) and, with --kmers, `<project>.kmx.txt` (the k-mers as letters, one per line).  The
tables are staged in HBM slice by slice (PK_MERGE_HBM_BUDGET) and selected, compacted and spelled on the GPU; one device
(PK_DEVICE).
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

from pykmer_amd.extract import main  # noqa: E402

if __name__ == "__main__":
    try:
        main()
    finally:
        _warm.join()           # an early `error: ...` exit must not tear the interpreter down inside the HIP start-up
