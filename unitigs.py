#!/usr/bin/env python3
"""unitigs.py Project_Name table.kin[.bgz] [--min-count A --max-count B] [--min-kmers M] [--gfa]

Builds the unitigs of ONE k-mer table (no counterpart in the reference: the BCALM step behind a k-mer count): the k-mers
whose count lies in the count window are the nodes of a de Bruijn graph, and the k-mers that overlap by k-1 bases without
ambiguity are joined into sequences on the GPU (README "Unitigs").  `<project>.unitigs.fa` holds one record per unitig,
named by its row index; `<project>.kmu` (np.savez_compressed: first_addr, n_kmers, depth, circular and the parameters) and
`<project>.kmu.json` record the run; `--gfa` adds `<project>.unitigs.gfa`, the unitigs and the edges between their ends.
Several tables are combined into one first with `extract.py --table`.  One device (PK_DEVICE).
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

from pykmer_amd.unitigs import main  # noqa: E402

if __name__ == "__main__":
    try:
        main()
    finally:
        _warm.join()           # an early exit (a refused argument) must not take the interpreter down under a HIP start-up in flight
