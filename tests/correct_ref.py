"""The yardstick of correct.py (README "Correcting reads"): the definition restated in plain Python on the references that
exist, independently of the kernels.

The FASTQ stands for a FASTA text (trim_ref.fasta_of: with a threshold the bases below it are N).  Positions are
mask_bed_ref.positions of that text, valid and covered bases mask_ref's, the line geometry trim_ref's.  Per record the valid
bases are laid out on their positions; a VALID RUN is a maximal stretch [lo, hi) of positions that all hold one; a CANDIDATE is
a valid base that is not covered and lies in a run with hi - lo >= k; its windows begin at max(lo, p - k + 1) .. min(p, hi - k).
A candidate with fewer than M windows is untried.  A base other than the read's own passes iff every window matches with it
at p -- the canonical address of a window is worked out here with Python integers (address), not taken from the oracle, and
tests/test_correct_host.py holds the two equal.  Exactly one passing base: corrected; two or three: ambiguous; none: unfixable.
Every candidate is judged against the uncorrected read.
"""
import numpy as np

import mask_bed_ref
import mask_ref
import trim_ref

FIELDS = ("pos2", "seq_len", "candidates", "untried", "corrected", "ambiguous")
CODE = {ord(c): i for i, c in enumerate("ACGT")}
CODE.update({ord(c): i for i, c in enumerate("acgt")})


def default_min_windows(k: int) -> int:
    return (k + 1) // 2


def address(codes) -> int:
    """The canonical address of a window given as base codes 0 .. 3: the smaller of the forward word (first base highest)
    and the word of the reverse complement."""
    fwd = rev = 0
    for c in codes:
        fwd = (fwd << 2) | c
    for c in reversed(codes):
        rev = (rev << 2) | (3 - c)
    return min(fwd, rev)


def _matches(tables, addrs, min_count, max_count) -> np.ndarray:
    addrs = np.array(addrs, dtype=np.uint64)
    hit = np.zeros(addrs.size, dtype=bool)
    for table in tables:
        c = np.asarray(table[addrs]).astype(np.int64)
        hit |= (c >= min_count) & (c <= max_count)
    return hit


def expected(fq: bytes, k: int, tables, min_count: int = 1, max_count: int = 255, M: int = None, T: int = 0, cover=None) -> dict:
    """dict of the six FIELDS and unfixable, (R,) uint64 each; fix_record, fix_pos (F,) uint64 and fix_old, fix_new (F,) uint8 in
    stream order; patched: the corrected bytes of fq; n_bases, cover (n_bases,) bool and bits (packed).  `tables`: dense u8
    arrays of 4^k bytes or query_ref.SparseTables.  M: None = (k + 1) // 2.  `cover`: (n_bases,) bools that stand in for the
    bits of the tables (bits from anywhere)."""
    fq = bytes(fq)
    M = default_min_windows(k) if M is None else M
    assert 1 <= M <= k
    geo = trim_ref.runs(fq, list(tables) if cover is None else np.asarray(cover, dtype=bool), k, min_count, max_count, T=T)
    fasta = trim_ref.fasta_of(fq, T)
    base_off, base_rec, _, _ = mask_ref.walk(fasta, 1)
    rec_of, pos_of = mask_bed_ref.positions(fasta)
    R = geo["seq_len"].size
    valid = [np.zeros(int(n), dtype=bool) for n in geo["seq_len"]]
    covered = [np.zeros(int(n), dtype=bool) for n in geo["seq_len"]]
    codes = [np.full(int(n), -1, dtype=np.int64) for n in geo["seq_len"]]
    for off, r, cov in zip(base_off.tolist(), base_rec.tolist(), geo["cover"].tolist()):
        p = int(pos_of[off])
        assert rec_of[off] == r and 0 <= p < valid[r].size
        valid[r][p], covered[r][p], codes[r][p] = True, cov, CODE[fasta[off]]
    out = {name: np.zeros(R, dtype=np.uint64) for name in FIELDS + ("unfixable",)}
    out["pos2"], out["seq_len"] = geo["pos2"].copy(), geo["seq_len"].copy()
    patched = bytearray(fq)
    fixes = []
    for r in range(R):
        n = valid[r].size
        lo = 0
        while lo < n:
            if not valid[r][lo]:
                lo += 1
                continue
            hi = lo
            while hi < n and valid[r][hi]:
                hi += 1
            for p in range(lo, hi):
                if covered[r][p] or hi - lo < k:
                    continue
                out["candidates"][r] += 1
                starts = list(range(max(lo, p - k + 1), min(p, hi - k) + 1))
                assert 1 <= len(starts) <= k
                if len(starts) < M:
                    out["untried"][r] += 1
                    continue
                own = int(codes[r][p])
                passing = []
                for b in range(4):
                    if b == own:
                        continue
                    addrs = []
                    for s in starts:
                        window = codes[r][s:s + k].tolist()
                        window[p - s] = b
                        addrs.append(address(window))
                    if bool(_matches(tables, addrs, min_count, max_count).all()):
                        passing.append(b)
                if len(passing) == 1:
                    out["corrected"][r] += 1
                    at = int(geo["pos2"][r]) + p
                    old = fq[at]
                    assert CODE[old] == own
                    new = b"ACGT"[passing[0]] | (old & 0x20)
                    patched[at] = new
                    fixes.append((r, p, old, new))
                elif passing:
                    out["ambiguous"][r] += 1
                else:
                    out["unfixable"][r] += 1
            lo = hi
    assert np.array_equal(out["candidates"], out["untried"] + out["corrected"] + out["ambiguous"] + out["unfixable"])
    out.update(fix_record=np.array([f[0] for f in fixes], dtype=np.uint64), fix_pos=np.array([f[1] for f in fixes], dtype=np.uint64),
               fix_old=np.array([f[2] for f in fixes], dtype=np.uint8), fix_new=np.array([f[3] for f in fixes], dtype=np.uint8),
               patched=bytes(patched), n_bases=geo["n_bases"], cover=geo["cover"], bits=mask_ref.pack(geo["cover"]),
               n_valid_bases=geo["n_valid_bases"])
    return out


def totals(want: dict) -> dict:
    """What Corrector.finish reports for the whole stream."""
    return {"n_records": int(want["seq_len"].size), "n_bases": int(want["n_bases"]), "n_candidates": int(want["candidates"].sum()),
            "n_untried": int(want["untried"].sum()), "n_corrected": int(want["corrected"].sum()), "n_ambiguous": int(want["ambiguous"].sum())}
