"""CPU: the query path's yardstick (query_ref), its file writers, its argument checks and its table grouping.
No call here touches a GPU: staging and streaming are stood in for by query_ref."""
import json
import types

import numpy as np
import pytest

import inputs
import oracle
import query_bins_ref
import query_pairs_ref
import query_ref
from host_support import stub_header
from oracle import pyoracle
from pykmer_amd import query


def test_query_ref_agrees_with_a_literal_restatement():
    """Pins the yardstick: per record, walk the windows the reference's gen_kmers yields and look each one up."""
    k, text = 5, inputs.edge_fasta()
    tables = query_ref.random_tables(k, 3, seed=50)
    for mn, mx in ((1, 255), (2, 254), (255, 255), (1, 1)):
        want = query_ref.expected(text, k, tables, mn, mx)
        recs = list(pyoracle.records(text.decode("utf-8")))
        assert len(recs) == want["hits"].shape[0] and len(recs) > 3
        assert query_ref.names(text, want["records"]) == [name for name, _, _ in recs]
        some_empty = False
        for r, (name, seq, seq_len) in enumerate(recs):
            canon = [min(f, v) for _, f, v in pyoracle.windows(seq, k)]
            assert len(canon) == int(want["n_valid"][r]) and seq_len == int(want["seq_len"][r])
            some_empty |= not canon
            for t, table in enumerate(tables):
                c = [int(table[a]) for a in canon]
                assert sum(1 for v in c if mn <= v <= mx) == int(want["hits"][r, t])
                assert sum(v for v in c if mn <= v <= mx) == int(want["depth"][r, t])
        assert some_empty                                    # records without a window are listed


def test_sparse_table_reads_like_the_dense_one():
    k = 5
    rng = np.random.default_rng(3)
    counted = rng.integers(0, 4 ** k, 700).astype(np.uint64)
    counted = np.concatenate([counted, np.full(300, 17, dtype=np.uint64)])      # one k-mer beyond 255
    dense = np.zeros(4 ** k, dtype=np.uint8)
    pyoracle.apply_batch(dense, counted)
    sparse = query_ref.SparseTable(counted)
    probe = np.arange(4 ** k, dtype=np.uint64)
    assert np.array_equal(sparse[probe], dense) and dense[17] == 255


def _result(R=5, N=3, seed=1):
    rng = np.random.default_rng(seed)
    n_valid = rng.integers(0, 1000, R).astype(np.uint64)
    n_valid[2] = 0
    hits = (rng.integers(0, 1001, (R, N)).astype(np.uint64) * n_valid[:, None]) // np.uint64(1000)
    return {"names": [f"rec {i} \t" if i == 1 else f"rec{i}" for i in range(R)], "seq_len": n_valid + np.uint64(8), "n_valid": n_valid,
            "hits": hits, "depth": hits * np.uint64(3), "kmer_len": 9, "min_count": 2, "max_count": 200}


def test_writers(tmp_path):
    res = _result()
    proj = str(tmp_path / "proj")
    data = [{"pos": i, "index_file": tmp_path / f"t{i}.kin", "description_file": tmp_path / f"t{i}.kin.json", "header": {"kmer_len": 9}}
            for i in range(3)]
    query.write_kmq(proj, res, "q.fa", data, ["ta", "tb", "tc"])
    assert not list(tmp_path.glob("*.tmp"))
    z = np.load(proj + ".kmq")
    assert sorted(z.files) == ["depth", "hits", "kmer_len", "max_count", "min_count", "n_valid", "seq_len"]
    for key, shape in (("hits", (5, 3)), ("depth", (5, 3)), ("n_valid", (5,)), ("seq_len", (5,))):
        assert z[key].dtype == np.uint64 and z[key].shape == shape and np.array_equal(z[key], res[key]), key
    assert (int(z["kmer_len"]), int(z["min_count"]), int(z["max_count"])) == (9, 2, 200)
    with open(proj + ".kmq.json") as fh:
        meta = json.load(fh)
    assert sorted(meta) == ["data", "kmer_len", "max_count", "min_count", "project_name", "query_file", "records"]
    assert meta["records"] == [n.strip() for n in res["names"]] and meta["query_file"] == "q.fa" and meta["project_name"] == proj
    assert [d["pos"] for d in meta["data"]] == [0, 1, 2] and meta["data"][1]["index_file"] == str(tmp_path / "t1.kin")
    lines = open(proj + ".kmq.tsv").read().split("\n")
    assert lines[0] == "record\tseq_len\tn_valid\tta\ttb\ttc" and lines[-1] == "" and len(lines) == 7
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert [r[0] for r in rows] == meta["records"]
    assert np.array_equal(np.array([[int(v) for v in r[3:]] for r in rows], dtype=np.uint64), res["hits"])
    assert [int(r[1]) for r in rows] == list(res["seq_len"]) and [int(r[2]) for r in rows] == list(res["n_valid"])
    with pytest.raises(ValueError, match="already exists"):
        query.query(proj, "q.fa", [tmp_path / "t0.kin"])


def test_argument_errors(tmp_path):
    a, b = stub_header(9, "a.kin"), stub_header(9, "b.kin")
    assert query.validate([a, b], 1, 255) == 9
    with pytest.raises(ValueError, match="c.kin.*differs"):
        query.validate([a, stub_header(11, "c.kin")], 1, 255)
    with pytest.raises(ValueError, match="even.kin"):
        query.validate([stub_header(8, "even.kin")], 1, 255)
    with pytest.raises(ValueError, match="deep.kin.*19"):
        query.validate([a, stub_header(19, "deep.kin")], 1, 255)
    for mn, mx in ((5, 4), (0, 3), (1, 256)):
        with pytest.raises(ValueError, match="count window"):
            query.validate([a], mn, mx)
    with pytest.raises(ValueError, match="at least one table"):
        query.validate([], 1, 255)
    with pytest.raises(ValueError, match="at least one table"):
        query.query_records("q.fa", [], 1, 255)
    # from files: a .kin.json that records an even kmer_len is reported with the file's name
    with pytest.raises(ValueError, match="nothing.kin"):
        query.load_header(tmp_path / "nothing.kin")
    with pytest.raises(ValueError, match="x.txt"):
        query.load_header(tmp_path / "x.txt")


def test_table_groups_concatenate_like_one_group():
    k, text = 5, inputs.edge_fasta()
    dense = query_ref.random_tables(k, 5, seed=51)
    tables = [types.SimpleNamespace(kmer_len=k, index_file=f"t{i}.kin", data_size=4 ** k, table=t) for i, t in enumerate(dense)]
    staged_sizes, freed = [], []

    def stage(group, device):
        staged_sizes.append(len(group))
        s = query.Staged([g.table for g in group])
        s.free = lambda: freed.append(len(group))
        return s

    def run(query_file, kmer_len, ptrs, mn, mx, device, first):
        want = query_ref.expected(text, kmer_len, ptrs, mn, mx)
        out = {key: want[key] for key in ("seq_len", "n_valid", "hits", "depth")}
        if first:
            out["names"] = query_ref.names(text, want["records"])
        return out

    one = query.query_records("q.fa", tables, 2, 254, hbm_budget=1 << 40, stage=stage, run=run)
    assert staged_sizes == [5] and one["n_groups"] == 1
    staged_sizes.clear()
    many = query.query_records("q.fa", tables, 2, 254, hbm_budget=2 * 4 ** k + 100, stage=stage, run=run)
    assert staged_sizes == [2, 2, 1] and many["n_groups"] == 3 and freed == [5, 2, 2, 1]
    tiny = query.query_records("q.fa", tables, 2, 254, hbm_budget=1, stage=stage, run=run)       # never fewer than one table
    assert tiny["n_groups"] == 5
    want = query_ref.expected(text, k, dense, 2, 254)
    for got in (one, many, tiny):
        assert got["hits"].shape == (len(want["records"]), 5) and got["names"] == query_ref.names(text, want["records"])
        for key in ("hits", "depth", "n_valid", "seq_len"):
            assert np.array_equal(got[key], want[key]), key
    assert query.table_groups(13, 1 << 30, 5 << 30) == [(0, 5), (5, 10), (10, 13)]


def _long_record_lies_late_in_the_first_chunk(text, index, s, ragged, k, tail_len=3000):
    chunk = 16384
    recs = oracle.kmer_list(text, k, records=True)[1]["records"]
    assert len(recs) == s + 2 and index == s
    long_, tail = recs[index], recs[index + 1]
    assert text[int(long_["name_off"]):int(long_["name_off"]) + int(long_["name_len"])] == b"long"
    assert int(long_["seq_len"]) == 12_000 and int(long_["n_valid_kmers"]) == 12_000 - k + 1
    end = int(tail["name_off"]) - 1                          # the '>' of the next record
    assert 0 < int(long_["name_off"]) < end < chunk < len(text) - 100 and int(tail["seq_len"]) == tail_len
    first_with_window = int(np.flatnonzero(recs["n_valid_kmers"] > 0)[0])
    assert first_with_window == 0 and index - first_with_window == s
    without = int(np.count_nonzero(recs["n_valid_kmers"][:s] == 0))
    assert without == (len(range(1, s, 3)) if ragged else 0)
    # bases of the chunk in front of the long record: all of them, or at least those of the reads that have a window
    for before in (int(recs["seq_len"][:s].sum()), int(recs["seq_len"][:s][recs["n_valid_kmers"][:s] > 0].sum())):
        assert (before + 12_000) // 1024 - -(-before // 1024) >= 2


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("s", [126, 127, 128, 129, 200])
def test_long_after_short_puts_a_long_record_late_in_the_first_chunk(s, ragged):
    """The builder of the GPU test of that name: the long record lies whole in the first 16 KiB chunk, it is record s
    counted from the chunk's first record with a window, and whole 1024-base waves of the chunk hold nothing else."""
    text, index = query_ref.long_after_short(s, seed=300 + s, ragged=ragged)
    _long_record_lies_late_in_the_first_chunk(text, index, s, ragged, 9)


def test_long_after_short_keeps_its_text_with_the_default_read_length():
    """read_len and source are additions: the texts of the k = 9 tests are what they were (sha256 of the earlier output)."""
    import hashlib
    got = [hashlib.sha256(query_ref.long_after_short(s, seed=300 + s, ragged=ragged)[0]).hexdigest()[:16]
           for s, ragged in ((20, True), (129, False), (200, True))]
    assert got == ["a3f4971c50518a04", "1dd3d68afaf709a2", "918bb3923bad0d6e"]


# ------------------------------------------------------------------ read-shaped input at k = 13, 15, 17
QACC_RECS, QSPEC_ROWS, QPAIR_ROWS = 128, 32, 64              # kmer_query.hip: the rows of a slot that are tallied in LDS


@pytest.mark.parametrize("k", [13, 15, 17])
def test_counted_sources_answer_every_count_window_differently(k):
    """Every table holds k-mers counted once, twice and to the clip, and every pair of tables shares some of each and not all."""
    sources, tables = query_ref.counted_case(k)
    assert len(sources) == query_ref.n_tables(k) and all(50_000 < len(query_ref.sequence(s)) < 70_000 for s in sources)
    for t in tables:
        for c in (1, 2, 255):                                # 255: the k + 3 k-mers of a tandem repeat's unit, in three repeats or four
            assert np.count_nonzero(t.vals == c) > (1000 if c < 255 else 2 * (k + 3)), c
    for i in range(len(tables)):
        for j in range(i + 1, len(tables)):
            both = np.intersect1d(tables[i].keys, tables[j].keys)
            ci, cj = tables[i][both], tables[j][both]
            for c in (1, 2, 255):
                n = np.count_nonzero((ci == c) & (cj == c))
                least = 1000 if c < 255 else k
                assert least < n <= min(np.count_nonzero(tables[i].vals == c), np.count_nonzero(tables[j].vals == c)) - least, (i, j, c)


@pytest.mark.parametrize("k,n_reads,fastq", [(13, 3000, False), (15, 3000, False), (17, 3000, False), (17, 5000, False),
                                             (15, 3000, True), (17, 3000, True), (15, 5000, True)])
def test_reads_from_gives_what_the_gpu_tests_rely_on(k, n_reads, fastq):
    """Seven chunks of reads: every length of read_lengths, reads without a window, several records in a thread's 16
    windows, and per table and count window hits that differ between the windows and between the tables of a pair."""
    sources, tables = query_ref.counted_case(k)
    text = query_ref.reads_case(k, n_reads, fastq)
    fmt = "fastq" if fastq else "fasta"
    if n_reads == 3000:
        assert 100_000 < len(query_ref.reads_case(k, n_reads, False)) < 7 * query_ref.CHUNK
    sums = {}
    for window in query_ref.COUNT_WINDOWS:
        want = query_pairs_ref.expected(text, k, tables, *window, fmt=fmt)
        n_valid, hits = want["n_valid"], want["hits"]
        assert len(want["records"]) == n_reads and (n_valid == 0).sum() > n_reads // 4 and (n_valid == 1).any()
        assert set(want["seq_len"].tolist()) == set(query_ref.read_lengths(k))
        assert 40_000 * n_reads // 3000 < int(n_valid.sum()) < 50_000 * n_reads // 3000
        sums[window] = hits.sum(axis=0)
        assert hits.any(axis=0).all() and (hits.sum(axis=1) == 0)[n_valid > 0].any()     # reads that hit and (random) reads that do not
        total = want["shared"].sum(axis=0)
        for p, (i, j) in enumerate(query_pairs_ref.pair_list(len(tables))):
            assert 0 < total[p] < min(sums[window][i], sums[window][j]), (window, i, j)
    for t in range(len(tables)):
        assert len({int(sums[w][t]) for w in query_ref.COUNT_WINDOWS}) == 3, t
    # more records with a window than any LDS accumulator has rows, in every chunk; N in every fifth read with a base
    fasta = query_ref.expected(text, k, tables, 1, 255, fmt)["fasta"]
    for c in range(0, len(fasta) - query_ref.CHUNK, query_ref.CHUNK):
        assert fasta[c:c + query_ref.CHUNK].count(b">") > 2 * QACC_RECS
    assert fasta.count(b"N") == (want["seq_len"] > 0).sum() // 5
    if fastq:
        from fastq_qual_ref import mask_fastq_to_fasta
        masked_text, n_masked = mask_fastq_to_fasta(text, 33 + 20)
        masked = query_pairs_ref.expected(masked_text, k, tables, 1, 255)
        plain = query_pairs_ref.expected(text, k, tables, 1, 255, fmt="fastq")
        assert n_masked > 1000 and int(plain["n_valid"].sum()) // 4 < int(masked["n_valid"].sum()) < 3 * int(plain["n_valid"].sum()) // 4
        assert masked["shared"].any(axis=0).all() and text.count(b"\r\n") == 4 * len(range(0, n_reads, 3))
    elif n_reads == 5000:
        assert text.count(b">") == 5000 > 4096               # one feed opens more records than the record array first holds


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("s", [QSPEC_ROWS - 1, QSPEC_ROWS, QSPEC_ROWS + 1, QPAIR_ROWS - 1, QPAIR_ROWS, QPAIR_ROWS + 1,
                               QACC_RECS - 1, QACC_RECS, QACC_RECS + 1])
def test_long_after_short_at_k17_puts_the_long_record_at_row_s(s, ragged):
    """read_len = k + 3 at k = 17: the asserts of the k = 9 builder hold, the reads have four windows, the long record hits
    both tables and shares windows between them under both count windows, and with bins of 5000 windows it has three rows
    of which, unragged, the first is row s of the slot."""
    k = 17
    text, index = query_ref.rows_case(s, ragged, k)
    _long_record_lies_late_in_the_first_chunk(text, index, s, ragged, k, tail_len=4000)
    tables = query_ref.counted_case(k)[1]
    for window in ((1, 255), (2, 254)):
        want = query_pairs_ref.expected(text, k, tables, *window)
        assert set(want["n_valid"][:index].tolist()) == ({0, 4} if ragged else {4})
        assert want["hits"][index].all() and want["shared"][index].all() and want["hits"][:index].any(axis=0).all()
        assert want["shared"][index, 0] < want["hits"][index].min()
    first, _, _, record, _ = query_bins_ref.bin_bounds(want["n_valid"], 5000)
    assert int(first[index + 1] - first[index]) == 3 and int(first[index]) == (s if not ragged else s - len(range(1, s, 3)))


@pytest.mark.parametrize("k", [13, 17])
def test_record_break_at_puts_the_break_d_bases_behind_the_chunk_boundary(k):
    """For every d: B's first base is valid base d of the second chunk, the text has two chunks, whole waves in front of the
    boundary lie in A, and the 2 k windows on either side of the break are counted once in every table."""
    chunk = query_ref.CHUNK
    tables = query_ref.counted_case(k)[1]
    is_base = np.zeros(256, dtype=bool)
    is_base[list(b"ACGT")] = True
    for d in range(-k, k + 1):
        text = query_ref.break_case(k, d)
        kmers, info = oracle.kmer_list(text, k, records=True)
        recs = info["records"]
        assert len(recs) == 2 and chunk + 2000 < len(text) < 2 * chunk
        b_first = int(recs[1]["name_off"]) + int(recs[1]["name_len"]) + 1         # behind the header's line end
        assert text[int(recs[1]["name_off"]) - 1:b_first] == b">B\n"
        if d >= 0:                                           # d bases of A open the second chunk; nothing else of it lies before B
            gap = np.frombuffer(text[chunk:b_first], dtype=np.uint8)
            assert int(is_base[gap].sum()) == d and (d == 0) == (b_first == chunk)
            assert (d == 0 or text[chunk:chunk + d].isalpha()) and int(recs[0]["name_off"]) < chunk
        else:                                                # -d bases of B close the first chunk
            assert b_first == chunk + d and text[b_first:chunk + 1].isalpha()
        n_a, n_b = int(recs[0]["n_valid_kmers"]), int(recs[1]["n_valid_kmers"])
        assert int(recs[1]["seq_len"]) == 2200 and n_b == 2200 - k + 1 and n_a == int(recs[0]["seq_len"]) - k + 1 > 15 * 1024
        for t in tables:
            assert (t[kmers[n_a - 2 * k:n_a + 2 * k]] == 1).all()
        assert np.count_nonzero(tables[0][kmers[:n_a]]) > n_a - 20 * k            # A but for the windows across its source's records


def test_the_row_limits_mirror_the_kernel():
    """QACC_RECS, QSPEC_ROWS and QPAIR_ROWS as this file and the GPU tests state them are kmer_query.hip's."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "pykmer_amd", "csrc", "kmer_query.hip")).read()
    kernel = tuple(int(re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1)) for name in ("QACC_RECS", "QSPEC_ROWS", "QPAIR_ROWS"))
    assert kernel == (QACC_RECS, QSPEC_ROWS, QPAIR_ROWS)
    reads = open(os.path.join(root, "tests", "test_gpu_query_reads.py")).read()
    assert tuple(int(v) for v in re.search(r"^QACC_RECS, QSPEC_ROWS, QPAIR_ROWS = (\d+), (\d+), (\d+)", reads, flags=re.M).groups()) == kernel
    pairs = open(os.path.join(root, "tests", "test_gpu_query_pairs.py")).read()
    assert int(re.search(r"^QPAIR_ROWS = (\d+)", pairs, flags=re.M).group(1)) == kernel[2]


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("s", [QPAIR_ROWS - 1, QPAIR_ROWS, QPAIR_ROWS + 1, 129, 200])
def test_long_after_short_for_the_pairs(s, ragged):
    """The builder of test_gpu_query_pairs.py::test_long_record_behind_short_ones, with its seed: the layout, and every
    pair of 16 random tables shares windows in every row of the long record under both of the test's count windows."""
    k = 9
    text, index = query_ref.long_after_short(s, seed=980 + s, ragged=ragged, tail_len=4000)
    _long_record_lies_late_in_the_first_chunk(text, index, s, ragged, k, tail_len=4000)
    tables = query_ref.random_tables(k, 16, 901)
    for window in ((1, 255), (255, 255)):
        for W in (None, 1000):
            want = query_pairs_ref.expected(text, k, tables, *window, W=W)
            rows = slice(index, index + 1) if W is None else slice(int(want["bin_first"][index]), int(want["bin_first"][index + 1]))
            assert want["shared"].shape[1] == 120 and want["shared"][rows].all() and rows.stop - rows.start == (1 if W is None else 12)
            assert W is None or ragged or rows.start == s
