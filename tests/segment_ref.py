"""Tables described as segments, and the merger's results on them in closed form.

A segment list is [(start, end, values), ...]: addresses [start, end) hold values[i] in table i, the segments cover
[0, n) without gaps, and a planted single byte is a segment of length 1.  Every result of the merge-side kernels is a sum
over segments of length x f(values), so it is computed here without a table ever being materialised -- which is what lets
a test state what tables of more than 2^32 bytes must give, and what a kernel that cuts an address to 32 bits (fold) or
to 31 bits (clip) would give instead."""
import numpy as np

from pykmer_amd import _lib, kwip, spectrum


# ------------------------------------------------------------------ segment lists
def check(segs, n=None):
    """The list covers [0, n) in order without gaps or empty segments; returns (n, N)."""
    at, N = 0, len(segs[0][2])
    for s, e, v in segs:
        assert s == at and e > s and len(v) == N, (s, e, at, len(v), N)
        assert all(0 <= int(x) <= 255 for x in v), v
        at = e
    assert n is None or at == n, (at, n)
    return at, N


def restrict(segs, lo, hi):
    """The content of [lo, hi) as a segment list that starts at 0."""
    return [(max(s, lo) - lo, min(e, hi) - lo, v) for s, e, v in segs if s < hi and e > lo]


def shifted(segs, by):
    return [(s + by, e + by, v) for s, e, v in segs]


def fold(segs, border):
    """What a kernel reads that cuts its addresses to log2(border) bits: address x holds the content of x mod border."""
    n, _ = check(segs)
    out, at = [], 0
    while at < n:
        out += shifted(restrict(segs, 0, min(border, n - at)), at)
        at += border
    return out


def clip(segs, border):
    """What a kernel reads whose addresses at or above `border` fall outside the table: they read 0."""
    n, N = check(segs)
    if n <= border:
        return list(segs)
    return restrict(segs, 0, border) + [(border, n, (0,) * N)]


def tables_of(segs, idx):
    """The segment list of the tables idx[0], idx[1], ... (a table may occur more than once: aliased buffers are equal tables)."""
    return [(s, e, tuple(v[i] for i in idx)) for s, e, v in segs]


def with_plants(blocks, plants):
    """A gap-free list of blocks with single bytes planted in it: plants = {address: values}."""
    out = []
    for s, e, v in blocks:
        at = s
        for x in sorted(a for a in plants if s <= a < e):
            if x > at:
                out.append((at, x, v))
            out.append((x, x + 1, tuple(plants[x])))
            at = x + 1
        if at < e:
            out.append((at, e, v))
    assert sum(1 for s, e, v in out if e - s == 1) >= len(plants)
    return out


def materialise(segs):
    """The tables themselves, one uint8 array each: for layouts small enough to hold."""
    n, N = check(segs)
    tabs = [np.zeros(n, dtype=np.uint8) for _ in range(N)]
    for s, e, v in segs:
        for i in range(N):
            tabs[i][s:e] = v[i]
    return tabs


def weights(segs):
    """(V, L): the distinct value vectors (U, N) int64 and the number of addresses that hold each (U,) as Python ints."""
    tot = {}
    for s, e, v in segs:
        v = tuple(int(x) for x in v)
        tot[v] = tot.get(v, 0) + (e - s)
    keys = sorted(tot)
    return np.array(keys, dtype=np.int64).reshape(len(keys), -1), [tot[k] for k in keys]


# ------------------------------------------------------------------ closed-form results
def pair(segs, windows):
    """(W, N, N) uint64: pair[w][i][j], i <= j, = addresses where tables i and j both lie in window w; 0 below the diagonal."""
    V, L = weights(segs)
    N = V.shape[1]
    out = np.zeros((len(windows), N, N), dtype=np.uint64)
    for w, (mn, mx) in enumerate(windows):
        ok = (V >= mn) & (V <= mx)
        for u, length in enumerate(L):
            on = np.flatnonzero(ok[u])
            for a, i in enumerate(on):
                out[w, i, on[a:]] += np.uint64(length)
    return out


def spectrum_acc(segs):
    """The flat accumulator of spectrum_device_accumulate, laid out as merge_ref.numpy_spectrum lays it out."""
    V, L = weights(segs)
    N = V.shape[1]
    acc = np.zeros(_lib.spectrum_words(N), dtype=np.uint64)
    hist, core = spectrum.split_accumulator(acc, N)
    pairs = spectrum.pair_list(N)
    for u, length in enumerate(L):
        for i in range(N):
            hist[i, V[u, i]] += np.uint64(length)
        for p, (i, j) in enumerate(pairs):
            if V[u, i] and V[u, j]:
                core[p, V[u, i] - 1, V[u, j] - 1] += np.uint64(length)
    return acc


def occgram_acc(segs):
    """The flat accumulator of occgram_device_accumulate, laid out as merge_ref.numpy_occgram lays it out."""
    V, L = weights(segs)
    N = V.shape[1]
    acc = np.zeros(_lib.occgram_words(N), dtype=np.uint64)
    occ_hist, lin, gram = kwip.split_accumulator(acc, N)
    iu = np.triu_indices(N)
    for u, length in enumerate(L):
        o = int((V[u] > 0).sum())
        occ_hist[o] += np.uint64(length)
        if o:
            lin[o - 1] += (V[u] * length).astype(np.uint64)                  # < 2^8 * 2^40: exact in int64
            gram[o - 1] += (np.outer(V[u], V[u])[iu] * length).astype(np.uint64)
    return acc


def bit_word(v, mn, mx):
    return sum(1 << t for t, x in enumerate(v) if mn <= x <= mx)


def patterns(segs, mn, mx):
    """(2^N,) uint64: the addresses per presence pattern under one window."""
    V, L = weights(segs)
    out = np.zeros(1 << V.shape[1], dtype=np.uint64)
    for u, length in enumerate(L):
        out[bit_word(V[u], mn, mx)] += np.uint64(length)
    return out


def selected(v, P, mn, mx, min_present, max_absent):
    """The extract condition on one value vector: the first P tables are the present ones."""
    p = sum(1 for x in v[:P] if mn <= x <= mx)
    q = sum(1 for x in v[P:] if x >= 1)
    return p >= min_present and q <= max_absent


def extract_count(segs, P, mn, mx, min_present, max_absent):
    return sum(e - s for s, e, v in segs if selected(v, P, mn, mx, min_present, max_absent))


def extract_rows(segs, P, mn, mx, min_present, max_absent, first_addr=0, limit=1 << 16):
    """(addr (M,) uint64 ascending, counts (M, P) uint8) of a sparse selection (at most `limit` addresses)."""
    m = extract_count(segs, P, mn, mx, min_present, max_absent)
    assert m <= limit, ("not a sparse selection", m)
    addr, counts = [], []
    for s, e, v in segs:
        if selected(v, P, mn, mx, min_present, max_absent):
            addr += range(first_addr + s, first_addr + e)
            counts += [list(v[:P])] * (e - s)
    return np.array(addr, dtype=np.uint64), np.array(counts, dtype=np.uint8).reshape(len(addr), P)


def table_value(v, P, op, mn, mx, min_present, max_absent):
    """One byte of the output table of `op` (README "Tables from tables")."""
    if not selected(v, P, mn, mx, min_present, max_absent):
        return 0
    inside = [int(x) for x in v[:P] if mn <= x <= mx]
    return {"sum": min(255, sum(inside)), "min": min(inside), "max": max(inside), "count": len(inside)}[op]


def table(segs, P, op, mn, mx, min_present, max_absent):
    """(segments of the one output table, its hist256 (256,) uint64)."""
    out = [(s, e, (table_value(v, P, op, mn, mx, min_present, max_absent),)) for s, e, v in segs]
    hist = np.zeros(256, dtype=np.uint64)
    for s, e, v in out:
        hist[v[0]] += np.uint64(e - s)
    return out, hist


def window_bytes(segs, lo, hi):
    """The bytes [lo, hi) of a one-table segment list."""
    return materialise(restrict(segs, lo, hi))[0]


# ------------------------------------------------------------------ the layout of the tests past 2^32 addresses
N_BASE = 13
POOL = (0, 1, 2, 3, 4, 5, 7, 50, 51, 127, 128, 200, 201, 253, 254, 255)     # the edges of every window the tests use, and both sides of 128
PLANT_POOL = (255, 0, 1, 128, 2, 254, 3, 127, 0, 9, 200, 0, 51, 4, 0, 129, 100, 0, 6)


def block_values(b, N=N_BASE):
    """Block b in table i holds POOL[(3 b + 5 i + 1) mod 16]: 3 and 5 are odd, so for b < 16 no two blocks agree in any
    table and a block holds every table a different value (one 0 at most)."""
    return tuple(POOL[(3 * b + 5 * i + 1) % 16] for i in range(N))


def plant_values(j, N=N_BASE):
    """Plant j: a vector with zeros at changing places, so that plants land in occupancy classes the blocks never reach."""
    return tuple(PLANT_POOL[(7 * j + 3 * i) % len(PLANT_POOL)] for i in range(N))


def layout(block_log2=29, tail=2 ** 22 + 37, group=1024, sparse_present=0):
    """(segments, n, plant addresses).  Eight blocks of 2^block_log2 bytes and a tail, each with block_values of its own,
    and single bytes planted around half the head (2^31 at full size), around its end (2^32), at both ends of the
    2 x `group` bytes centred on it and of the word groups beside it, at block borders and at n - 38 and n - 1.
    sparse_present = P: the blocks hold 0 in the first P tables, so of those tables only the plants are left."""
    block = 1 << block_log2
    border = 8 * block
    half = border // 2
    n = border + tail
    assert tail > 2 * group + 2 and block > 4 * group
    blocks = [(b * block, min((b + 1) * block, n), block_values(b)) for b in range(8)] + [(border, n, block_values(8))]
    if sparse_present:
        blocks = [(s, e, (0,) * sparse_present + v[sparse_present:]) for s, e, v in blocks]
    at = [half - 1, half, border - 1, border, border + 1, border - group, border + group - 1, border - 2 * group, border + 2 * group - 1,
          n - 38, n - 1, 0, block - 1, block, 3 * block, 5 * block - 1, 7 * block + 5, half + group + 3, 17, 2 * group - 1, group,
          border + tail // 2, 6 * block + 2 * group, half - 2 * group]
    assert len(set(at)) == len(at) and all(0 <= x < n for x in at), at
    plants = {x: plant_values(j) for j, x in enumerate(at)}
    if sparse_present:                 # plants that can select: counts in the present tables, zeros in two of three plants behind them
        P = sparse_present
        plants = {x: tuple(v[i] or (2 + (i + j) % 3) for i in range(P)) + tuple(v[i] if (i + j) % 3 == 0 else 0 for i in range(P, len(v)))
                  for j, (x, v) in enumerate(plants.items())}
    segs = with_plants(blocks, plants)
    check(segs, n)
    return segs, n, sorted(at)


SMALL = dict(block_log2=9, tail=2 ** 2 + 37, group=8)        # the layout at 1/2^20: blocks of 2^9, borders at 2^11 and 2^12


# what the tests past 2^32 run, shared with the host test that keeps their preconditions from being vacuous
PAIR_RUNS = ((13, ((1, 255), (3, 200))), (41, ((2, 254),)))                       # gram_device_partial: N, windows
SWEEP_WINDOWS = ((1, 255), (2, 255), (3, 200), (4, 254), (5, 127), (128, 255), (1, 50), (2, 3))   # five of them at N = 17
SWEEP_RUNS = ((8, 8), (13, 8), (17, 5))                                           # N, windows in the one k_gram_mw pass
OCC_RUNS = (13, 17)
PATTERN_RUNS = ((13, ((1, 255), (3, 50))), (15, ((1, 255), (3, 50))))
EXTRACT = dict(tables=(0, 1, 2, 3, 7), P=3, A=2, mn=2, mx=200, min_present=2, max_absent=1)   # selects blocks 0 and 4: one on either side of 2^31


def aliased(N):
    """Table i of N reads buffer i mod 13."""
    return [i % N_BASE for i in range(N)]


def results(segs, sparse):
    """Every result the tests past 2^32 check, keyed by what produced it, for the 13-table layout `segs` and its sparse
    variant `sparse` (extract_rows): the references of the true layout, and of what a truncating kernel would read."""
    out = {}
    for N, windows in PAIR_RUNS:
        for w, m in zip(windows, pair(tables_of(segs, aliased(N)), windows)):
            out["pair", N, w] = m
    for N, W in SWEEP_RUNS:
        for w, m in zip(SWEEP_WINDOWS[:W], pair(tables_of(segs, aliased(N)), SWEEP_WINDOWS[:W])):
            out["sweep", N, w] = m
    out["spectrum", N_BASE] = spectrum_acc(segs)
    for N in OCC_RUNS:
        out["occgram", N] = occgram_acc(tables_of(segs, aliased(N)))
    for N, windows in PATTERN_RUNS:
        for w in windows:
            out["patterns", N, w] = patterns(tables_of(segs, aliased(N)), *w)
    e = EXTRACT
    five, cond = e["tables"], (e["P"], e["mn"], e["mx"], e["min_present"], e["max_absent"])
    out["extract", "dense"] = np.array([extract_count(tables_of(segs, five), *cond)], dtype=np.uint64)
    addr, counts = extract_rows(tables_of(sparse, five), *cond)
    out["extract", "addr"], out["extract", "counts"] = addr, counts
    for op in ("sum", "min", "max", "count"):
        out["table", op] = table(tables_of(segs, five), e["P"], op, *cond[1:])[1]
    return out


def assert_visible(true, other, what):
    """The precondition of a test past 2^32: the truncated layout `other` changes every result, in every tested window,
    and every table's part of every per-table output."""
    for key in true:
        a, b = true[key], other[key]
        assert a.shape != b.shape or not np.array_equal(a, b), (what, key)
    for kind, runs in (("pair", PAIR_RUNS), ("sweep", SWEEP_RUNS)):
        for N, _ in runs:
            d = sum((true[k] != other[k]).astype(np.int64) for k in true if k[:2] == (kind, N))
            assert all(d[i, :].any() or d[:, i].any() for i in range(N)), (what, kind, N)
    h0, h1 = (spectrum.split_accumulator(r["spectrum", N_BASE], N_BASE)[0] for r in (true, other))
    assert (h0 != h1).any(axis=1).all(), (what, "spectrum hist")
    for N in OCC_RUNS:
        l0, l1 = (kwip.split_accumulator(r["occgram", N], N)[1] for r in (true, other))
        assert (l0 != l1).any(axis=0).all(), (what, "occgram lin", N)


# ------------------------------------------------------------------ tables that meet every threshold everywhere
def threshold_tables(N, n=1 << 19, seed=0):
    """N tables of n bytes (a multiple of 2^19) in which every byte value occurs at every offset of a 2 KiB word group:
    a table is rows of 2048 bytes, and down each of the 2048 columns of 256 rows runs a random permutation of 0 .. 255,
    drawn independently per table, so pairs of tables meet every threshold from both sides."""
    assert n % (256 * 2048) == 0
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(N):
        parts = [rng.permuted(np.tile(np.arange(256, dtype=np.uint8)[:, None], (1, 2048)), axis=0) for _ in range(n // (256 * 2048))]
        out.append(np.concatenate(parts).reshape(-1))
    return out


def threshold_windows():
    """(t, 255), (1, t) and (t, t) for every t = 1 .. 255: three lists of 255 windows."""
    ts = range(1, 256)
    return [(t, 255) for t in ts], [(1, t) for t in ts], [(t, t) for t in ts]
