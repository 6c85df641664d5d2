"""The yardstick of the table output of the extract path: the definition (README "Tables from tables") on whole numpy
arrays, built on extract_ref.select_mask."""
import numpy as np

import extract_ref

OPS = ("sum", "min", "max", "count")


def expected(present, absent, op, min_count=1, max_count=255, min_present=None, max_absent=0):
    """(n,) uint8: 0 where an address is not selected, else `op` over V(x) = the present bytes inside the window."""
    T = np.stack([np.asarray(t) for t in present]).astype(np.int64)
    V = (T >= min_count) & (T <= max_count)
    if op == "sum":
        r = np.minimum(255, np.where(V, T, 0).sum(axis=0))
    elif op == "min":
        r = np.where(V, T, 256).min(axis=0)
    elif op == "max":
        r = np.where(V, T, 0).max(axis=0)
    elif op == "count":
        r = V.sum(axis=0)
    else:
        raise ValueError(op)
    sel = extract_ref.select_mask([np.asarray(t) for t in present], [np.asarray(t) for t in absent], min_count, max_count, min_present, max_absent)
    out = np.where(sel, r, 0)
    assert out.min() >= 0 and out.max() <= 255 and (out[sel] >= 1).all()     # a selected address has a byte in the window
    return out.astype(np.uint8)


def profile(present, absent, min_count=1, max_count=255, min_present=None, max_absent=0):
    """What a set of inputs exercises: dict(selected, saturated, unsaturated -- selected addresses whose unclamped sum is
    above / at most 255 --, mixed -- selected addresses where min != max --, occupancies -- the set of |V| over them)."""
    T = np.stack([np.asarray(t) for t in present]).astype(np.int64)
    V = (T >= min_count) & (T <= max_count)
    sel = extract_ref.select_mask(list(present), list(absent), min_count, max_count, min_present, max_absent)
    raw = np.where(V, T, 0).sum(axis=0)
    lo, hi = np.where(V, T, 256).min(axis=0), np.where(V, T, 0).max(axis=0)
    return {"selected": int(sel.sum()), "saturated": int((sel & (raw > 255)).sum()), "unsaturated": int((sel & (raw <= 255)).sum()),
            "mixed": int((sel & (lo != hi)).sum()), "occupancies": set(V.sum(axis=0)[sel].tolist())}


def hist256(table):
    return np.bincount(np.asarray(table, dtype=np.uint8), minlength=256).astype(np.uint64)
