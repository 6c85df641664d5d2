"""Numpy restatement of the presence patterns of a set of tables: the `partial_fn` stand-in of the CPU tests and the
yardstick of the GPU ones."""
import numpy as np


def bit_words(tabs, mn, mx) -> np.ndarray:
    """m(x) per address: bit t set where mn <= tabs[t][x] <= mx; a loop over the tables."""
    m = np.zeros(np.asarray(tabs[0]).size, dtype=np.int64)
    for t, tab in enumerate(tabs):
        tab = np.asarray(tab)
        m |= ((tab >= mn) & (tab <= mx)).astype(np.int64) << t
    return m


def numpy_patterns(tabs, mn, mx) -> np.ndarray:
    """(2^N,) u64: the addresses per bit word."""
    return np.bincount(bit_words(tabs, mn, mx), minlength=1 << len(tabs)).astype(np.uint64)


def numpy_patterns_partial(headers, lo, hi, windows, device, threads) -> np.ndarray:
    """The flat W x 2^N accumulator of merger.patterns_partial for addresses [lo, hi)."""
    tabs = [h.read_table_slice(lo, hi) for h in headers]      # a rank reads its slice of every file, nothing else
    return np.concatenate([numpy_patterns(tabs, mn, mx) for mn, mx in windows])
