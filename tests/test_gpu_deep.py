"""GPU parity of the deep-window kernel variant (k = 19 and 21: k_walk_sort<..., DEEP>, kmer_fuse.hip): windows cut from 96
bits, the 64-bit restart smear, and -- for a carried run of more than 16 bases -- the bases in front of a slot gathered
from the slots before it and, in front of a feed's first slots, from the feeds before it (Carry::deep_in).  k = 17 in two
slices runs next to them as the control that takes the ordinary 64-bit path.

Reference everywhere: tests/slice_ref.py (the one-shot oracle of the whole text, selected by address slice); all
comparisons are exact.  No case picks its slice blindly: the slice is the one that holds the canonical k-mer of the window
a case is about -- for a seam, the window that crosses it and reaches furthest back, which is the first to go wrong when
history is lost -- and the case asserts that from the oracle before anything runs on the GPU."""
import numpy as np
import pytest

import fastq_ref
import inputs
import slice_ref

pytestmark = pytest.mark.gpu

N_SLICES = slice_ref.N_SLICES
CHUNK = 16384


def _run(ix, exp, s, feeds, tag, full_table=False, name_off=None):
    ix.reset()
    for f in feeds:
        ix.feed(f)
    return exp.check(ix, s, full_table, tag, name_off)


def _cut(data, cuts):
    cuts = [0] + sorted(cuts) + [len(data)]
    return [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


# ------------------------------------------------------------------ 1. k = 21, real slices ---------------------------
def test_k21_real_slices(gpu):
    """k = 21 in 256 slices of 2^34 addresses: the first slice (poly-A saturates address 0), the last (k-mer and reverse
    complement both begin TTTT), the busiest other one, two seeded interior ones, and one that the oracle says stays empty
    (of the same text without its synthetic body: a few hundred kbp reach all 256 slices).
    Totals and records are whole-input figures and must be the same in every slice."""
    k, n = 21, 256
    data = inputs.deep_k21_fasta()
    assert 300_000 < len(data) < 1_000_000
    exp = slice_ref.Expect(data, k, n)
    distinct = exp.distinct_per_slice()
    assert distinct[0] > 0 and distinct[255] > 0, "the text was built to reach the first and the last slice"
    assert exp.u[0] == 0 and exp.sat[0] == 255, "poly-A saturates address 0"
    assert exp.slice(255)[1].max() == 255, "the planted top-slice k-mer saturates"
    busiest = exp.busiest(exclude=(0, 255))
    rng = np.random.default_rng(21)
    inner = [s for s in np.flatnonzero(distinct) if s not in (0, 255, busiest)]
    interior = sorted(int(s) for s in rng.choice(inner, size=2, replace=False))
    # an empty slice: a text of this size reaches all 256, so that case runs on the same text without its synthetic body
    small = slice_ref.Expect(inputs.deep_k21_fasta(body_bp=0), k, n)
    empty = [int(s) for s in np.flatnonzero(small.distinct_per_slice() == 0)]
    assert empty and small.distinct_per_slice()[0] > 0, "no empty slice: the empty-table case has nothing to run on"
    for s in (0, 255, busiest, *interior):
        assert distinct[s] > 0
        with gpu.Indexer(k, slice_index=s, n_slices=n) as ix:
            _run(ix, exp, s, [data], ("k21", s), full_table=s in (0, 255, busiest))
    s = empty[-1]
    with gpu.Indexer(k, slice_index=s, n_slices=n) as ix:
        fin = _run(ix, small, s, [small.data], ("k21 empty", s))
        assert int(fin["hist256"][0]) == 1 << 34 and int(fin["hist256"][1:].sum()) == 0
        part = np.empty(slice_ref.GIB, dtype=np.uint8)
        for off in range(0, 1 << 34, slice_ref.GIB):
            ix.table_slice_to_host(part, off)
            assert int(np.count_nonzero(part)) == 0, (s, off)


def test_k21_slice_arguments(gpu):
    with pytest.raises(ValueError):
        gpu.Indexer(21)                                        # 4 TiB: needs slices
    with pytest.raises(ValueError):
        gpu.Indexer(21, slice_index=0, n_slices=128)           # 2^35 addresses per slice
    with pytest.raises(ValueError):
        gpu.Indexer(21, slice_index=256, n_slices=256)
    with pytest.raises(ValueError):
        gpu.Indexer(23, slice_index=0, n_slices=4096)          # beyond the device path
    with gpu.Indexer(21, slice_index=255, n_slices=256) as ix:
        assert ix.finish()["hist256"][0] == 1 << 34


# ------------------------------------------------------------------ 2. slot seams inside one feed --------------------
def _site_crossing(kind, d, k):
    """How many windows cross a site of inputs.deep_seam_fasta: the carried run there, capped at k - 1."""
    if kind in ("N", "header"):
        return min(d, k - 1)
    return 0 if kind == "long_header" else k - 1


def _check_sites(exp, sites):
    """site -> slice of its furthest-reaching window, after asserting that the text carries the run the site is meant to."""
    need = {}
    for kind, d, off in sites:
        assert slice_ref.crossing_windows(exp.data, exp.k, off) == _site_crossing(kind, d, exp.k), (kind, d, off)
        need[(kind, d, off)] = {slice_ref.seam_slice(exp, off)}
    return need


@pytest.mark.parametrize("k", [17, 19, 21])
def test_slot_seams_in_one_feed(gpu, k):
    """One feed whose 16 KiB slot boundaries meet a carried run of every length 0 .. k + 3 (restart by N, restart by a
    header line) and the shapes that make the history gather walk: empty chunks, chunks with a few bases between empty
    ones, a header longer than two chunks, one-base lines, CR LF.  The sites sit at consecutive boundaries, so they fall
    on every place of a persistent workgroup's slot range, its first slot included.  k = 19, 21: the text is padded to
    >= 1024 chunks, so the sampling launch (COUNT, wave stretches, stride 16) runs the same code before the sort does;
    k = 17 (the control) stays below and is laid out exactly."""
    n = N_SLICES[k]
    data, sites = inputs.deep_seam_fasta(k, seed=200 + k, pad_to_chunks=1040 if k > 17 else 0)
    assert (len(data) >= 1024 * CHUNK) == (k > 17)
    exp = slice_ref.Expect(data, k, n)
    boundary_sites = [s for s in sites if s[0] != "line"]
    assert {(kind, d) for kind, d, _ in boundary_sites} >= {(kind, d) for kind in ("N", "header") for d in range(k + 4)}
    assert all(off % CHUNK == 0 for kind, _, off in boundary_sites if kind != "long_header")
    by_slice = slice_ref.cover(_check_sites(exp, boundary_sites))
    busiest = exp.busiest()
    for s in sorted(set(by_slice) | {busiest}):
        with gpu.Indexer(k, slice_index=s, n_slices=n) as ix:
            _run(ix, exp, s, [data], (k, s, by_slice.get(s)), full_table=s == busiest)
            assert ix.timings()["feeds"] == 1


# ------------------------------------------------------------------ 3. feed seams -----------------------------------
_PLAIN_BP = 3_400_000
_PIECE = 1 << 20


def _plain_text(k):
    """(text, N-restart cuts by d, cuts for short middle feeds, library piece cuts)"""
    n_cuts = {d: 100_000 + 4000 * d + 1 + d for d in range(k + 4)}            # d bases behind the N at 100 000 + 4000 d
    mid = {m: 400_000 + 1000 * m for m in (1, 5, 15, 16, 17)}                 # a feed of m bases ends here
    pieces = [_PIECE, 2 * _PIECE, 3 * _PIECE]
    empty_cut = 500_000
    motif_at = [cut - min(d, k - 1) for d, cut in n_cuts.items()] + [c - (k - 1) for c in (*mid.values(), *pieces, empty_cut)]
    text = inputs.plain_sequence_fasta(_PLAIN_BP, seed=300 + k, n_at=[cut - d - 1 for d, cut in n_cuts.items()], motif_at=motif_at)
    assert len(text) > 3 * _PIECE
    return text, n_cuts, mid, pieces, empty_cut


@pytest.mark.parametrize("k", [17, 19, 21])
def test_feed_seams(gpu, k, monkeypatch):
    """Feeds may end anywhere.  The slot-seam text and a 3.4 Mbp sequence on one line, each fed one-shot and then cut:
    d bases behind a restart (N, header) and behind a line start inside a run, d = 0 .. k + 3; at every other site of
    the slot-seam text; with a middle feed of 1 .. 17 bases, an empty one, one of line terminators only and one of
    blanks only; one byte at a time around a seam; at 40 seeded places; and by the library itself (PK_FEED_PIECE).
    A run of more than 16 bases across the seam needs bases that the carried state's 32 bits do not hold."""
    n = N_SLICES[k]
    seam_text, sites = inputs.deep_seam_fasta(k, seed=200 + k)
    seam = slice_ref.Expect(seam_text, k, n)
    plain_text, n_cuts, mid, pieces, empty_cut = _plain_text(k)
    plain = slice_ref.Expect(plain_text, k, n)
    cases = {}                                               # tag -> (expectation, feeds, PK_FEED_PIECE or None)
    need = {}

    def add(tag, exp, feeds, slices, piece=None):
        assert b"".join(feeds) == exp.data
        cases[tag] = (exp, feeds, piece)
        need[tag] = set(slices)

    for site, slices in _check_sites(seam, sites).items():
        kind, d, off = site
        add(("seam text", kind, d), seam, _cut(seam_text, [off]), slices)
        if kind in ("newlines", "blanks"):                   # the chunk in front of the site as a feed of its own
            assert set(seam_text[off - CHUNK:off]) <= set(b"\n ")
            add(("seam text", kind, "alone"), seam, _cut(seam_text, [off - CHUNK, off]), slices)
    deep_site = next(off for kind, d, off in sites if kind == "N" and d == k - 1)
    add(("seam text", "bytewise"), seam, _cut(seam_text, range(deep_site - 32, deep_site + 33)), {slice_ref.seam_slice(seam, deep_site)})
    rng = np.random.default_rng(40 + k)
    random_cuts = sorted(set(rng.integers(1, len(seam_text), size=40).tolist()))
    add(("seam text", "random"), seam, _cut(seam_text, random_cuts), {slice_ref.seam_slice(seam, c) for c in random_cuts})
    for d, cut in n_cuts.items():
        assert plain_text[cut - d - 1] == ord("N") and slice_ref.crossing_windows(plain_text, k, cut) == min(d, k - 1)
        add(("plain", "N", d), plain, _cut(plain_text, [cut]), {slice_ref.seam_slice(plain, cut)})
    for m, cut in mid.items():                               # the window that ends behind the short feed begins two feeds back
        assert slice_ref.crossing_windows(plain_text, k, cut) == k - 1
        add(("plain", "middle feed", m), plain, _cut(plain_text, [cut - m, cut]), {slice_ref.seam_slice(plain, cut)})
    add(("plain", "empty feed"), plain, [plain_text[:empty_cut], b"", plain_text[empty_cut:]], {slice_ref.seam_slice(plain, empty_cut)})
    add(("plain", "library pieces"), plain, [plain_text], {slice_ref.seam_slice(plain, pieces[0])}, piece=_PIECE)
    by_slice = slice_ref.cover(need)
    for s in sorted(by_slice):
        with gpu.Indexer(k, slice_index=s, n_slices=n) as ix:
            for exp in (seam, plain):                        # the control: the same text in one feed
                _run(ix, exp, s, [exp.data], (k, s, "one shot"))
            for tag in by_slice[s]:
                exp, feeds, piece = cases[tag]
                if piece:
                    monkeypatch.setenv("PK_FEED_PIECE", str(piece))
                _run(ix, exp, s, feeds, (k, s, tag))
                monkeypatch.delenv("PK_FEED_PIECE", raising=False)
                want_feeds = sum(1 for f in feeds if len(f)) if not piece else 3
                assert ix.timings()["feeds"] >= want_feeds, tag


@pytest.mark.parametrize("k", [19, 21])
def test_fastq_feed_seams(gpu, k):
    """FASTQ: the front end turns every feed into FASTA text and counts that text piece by piece, so a FASTQ feed that ends
    inside a read is a feed seam of the pipeline inside a run.  Reads of 320 bp, cut d bases into a read."""
    n = N_SLICES[k]
    rng = np.random.default_rng(500 + k)
    ds = (0, 5, 16, 17, k - 1, k + 3)
    fq, fa, cut_fq, cut_fa, names_at = [], [], {}, {}, []
    for r in range(40):
        seq = bytearray(inputs._rand_bases(rng, 320))
        d = ds[r // 5] if r % 5 == 2 and r // 5 < len(ds) else None
        name = b"read%d len=320" % r
        if d is not None:
            at = max(0, d - (k - 1))
            seq[at:at + len(inputs.SEAM_MOTIF)] = inputs.SEAM_MOTIF
            cut_fq[d] = sum(map(len, fq)) + len(name) + 2 + d
            cut_fa[d] = sum(map(len, fa)) + len(name) + 2 + d
        qual = bytes(rng.integers(33, 74, 320, dtype=np.uint8))
        names_at.append(sum(map(len, fq)) + 1)               # a FASTQ indexer reports the name where it lies in the FASTQ
        fq.append(b"@" + name + b"\n" + bytes(seq) + b"\n+\n" + qual + b"\n")
        fa.append(b">" + name + b"\n" + bytes(seq) + b"\n")
    fq, fa = b"".join(fq), b"".join(fa)
    assert fastq_ref.fastq_to_fasta(fq) == fa and sorted(cut_fq) == sorted(set(ds))
    exp = slice_ref.Expect(fa, k, n)
    names_at = np.array(names_at, dtype=np.uint64)
    assert all(fq[int(a):int(a) + int(ln)] == fa[int(o):int(o) + int(ln)]
               for a, o, ln in zip(names_at, exp.want["records"]["name_off"], exp.want["records"]["name_len"]))
    need = {}
    for d in cut_fq:
        assert slice_ref.crossing_windows(fa, k, cut_fa[d]) == min(d, k - 1)
        need[d] = {slice_ref.seam_slice(exp, cut_fa[d])}
    for s, cuts in sorted(slice_ref.cover(need).items()):
        with gpu.Indexer(k, slice_index=s, n_slices=n, fmt="fastq") as ix:
            _run(ix, exp, s, [fq], (k, s, "one shot"), name_off=names_at)
            for d in cuts:
                _run(ix, exp, s, _cut(fq, [cut_fq[d]]), (k, s, "cut", d), name_off=names_at)
            _run(ix, exp, s, _cut(fq, [cut_fq[d] for d in cuts]), (k, s, "all cuts"), name_off=names_at)


# ------------------------------------------------------------------ 4. repeats, overflow, wrap, reuse ----------------
@pytest.mark.parametrize("k", [19, 21])
def test_deep_tandem_repeats(gpu, k):
    """Tandem runs of period 1-3 and k - 2 .. k + 40 bases at every offset of a code word and across slot boundaries, an N in
    every seventh, and long A / AT / AAG / ACGT runs: the repeat test with `k & 16` and history from pprev0, the hot-key
    tallies and the side list.  Slice 0 (poly-A / poly-T, full table) and the busiest other slice."""
    n = N_SLICES[k]
    data = inputs.deep_tandem_fasta(k, seed=600 + k)
    assert len(data) > 30 * CHUNK
    exp = slice_ref.Expect(data, k, n)
    assert exp.u[0] == 0 and exp.sat[0] == 255, "poly-A saturates address 0"
    other = exp.busiest(exclude=(0,))
    assert int((exp.slice(other)[1] == 255).sum()) >= 1 or int((exp.sat == 255).sum()) >= 4
    for s in (0, other):
        with gpu.Indexer(k, slice_index=s, n_slices=n) as ix:
            _run(ix, exp, s, [data], (k, s), full_table=s == 0)
            cut = len(data) // 2 + 7                         # and the same in two feeds: tallies on top of a table that is not fresh
            _run(ix, exp, s, _cut(data, [cut]), (k, s, "two feeds"))


@pytest.mark.parametrize("k", [19, 21])
def test_deep_relayout_on_both_feeds(gpu, k):
    """Two texts that defeat the bucket sample, on one sliced indexer: both feeds take the exact re-layout, the second one on
    a table that is no longer fresh (test_bucket_overflow_takes_the_exact_relayout at deep k)."""
    n = N_SLICES[k]
    first = inputs.skewed_fasta(20_000_040, 61, seed=68, stretch=1024)
    more = inputs.skewed_fasta(18_000_000, 63, seed=11, stretch=1024)
    assert len(first) >= 1024 * CHUNK and len(more) >= 1024 * CHUNK
    exp = slice_ref.Expect(first + more, k, n)
    s = exp.busiest()
    with gpu.Indexer(k, slice_index=s, n_slices=n) as ix:
        ix.feed(first)
        one = ix.timings()["relayouts"]
        assert one >= 1, "the skewed text was meant to overflow the sampled layout"
        ix.feed(more)
        assert ix.timings()["relayouts"] > one
        exp.check(ix, s, tag=(k, s))


@pytest.mark.parametrize("k", [19, 21])
def test_deep_byte_counters_wrap(gpu, k):
    """A unit repeated 400 times, never in tandem, in the slice that holds most of its k-mers: its byte counters wrap and the
    buckets are counted again (test_byte_counters_wrap_and_are_recounted at deep k), on both feeds."""
    n = N_SLICES[k]
    copies = 400
    data = inputs.interspersed_repeat(copies, 70, 5000, seed=k)
    once = slice_ref.Expect(data, k, n)
    twice = slice_ref.Expect(data + data, k, n)
    u, c = np.unique(once.kmers, return_counts=True)
    repeated = np.bincount((u[c >= copies] // np.uint64(once.size)).astype(np.int64), minlength=n)
    s = int(repeated.argmax())                               # the slice that holds most of the unit
    assert repeated[s] >= 1 and repeated.sum() >= 70 - k + 1
    with gpu.Indexer(k, slice_index=s, n_slices=n) as ix:
        for feed in (1, 2):
            ix.feed(data)
            assert ix.timings()["buckets_recounted"] >= feed
        twice.check(ix, s, tag=(k, s))


def test_k21_reuse_after_reset(gpu):
    """One k = 21 slice indexer, reset between a large, a tiny, an empty and a large input: nothing leaks."""
    import synth
    k, n = 21, 256
    big = synth.c2(3_000_000, seed=21)[0].tobytes()
    again = synth.c2(2_000_000, seed=23)[0].tobytes()
    tiny = b">t\nACGTACGTTTGACCATTGACAGGATACCA\n"
    s = slice_ref.Expect(big, k, n).busiest()
    with gpu.Indexer(k, slice_index=s, n_slices=n) as ix:
        for data in (big, tiny, b"", again, big):
            exp = slice_ref.Expect(data, k, n)
            if data in (big, again):
                assert exp.distinct_per_slice()[s] > 0
            _run(ix, exp, s, [data] if data else [], (k, s, len(data)))
