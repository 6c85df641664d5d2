"""CPU: the query path's yardstick (query_ref), its file writers, its argument checks and its table grouping.
No call here touches a GPU: staging and streaming are stood in for by query_ref."""
import json
import types

import numpy as np
import pytest

import inputs
import query_ref
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


def _stub(k, name):
    return types.SimpleNamespace(kmer_len=k, index_file=name, data_size=4 ** k)


def test_argument_errors(tmp_path):
    a, b = _stub(9, "a.kin"), _stub(9, "b.kin")
    assert query.validate([a, b], 1, 255) == 9
    with pytest.raises(ValueError, match="c.kin.*differs"):
        query.validate([a, _stub(11, "c.kin")], 1, 255)
    with pytest.raises(ValueError, match="even.kin"):
        query.validate([_stub(8, "even.kin")], 1, 255)
    with pytest.raises(ValueError, match="deep.kin.*19"):
        query.validate([a, _stub(19, "deep.kin")], 1, 255)
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


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("s", [126, 127, 128, 129, 200])
def test_long_after_short_puts_a_long_record_late_in_the_first_chunk(s, ragged):
    """The builder of the GPU test of that name: the long record lies whole in the first 16 KiB chunk, it is record s
    counted from the chunk's first record with a window, and whole 1024-base waves of the chunk hold nothing else."""
    import oracle
    k, chunk = 9, 16384
    text, index = query_ref.long_after_short(s, seed=300 + s, ragged=ragged)
    recs = oracle.kmer_list(text, k, records=True)[1]["records"]
    assert len(recs) == s + 2 and index == s
    long_, tail = recs[index], recs[index + 1]
    assert text[int(long_["name_off"]):int(long_["name_off"]) + int(long_["name_len"])] == b"long"
    assert int(long_["seq_len"]) == 12_000 and int(long_["n_valid_kmers"]) == 12_000 - k + 1
    end = int(tail["name_off"]) - 1                          # the '>' of the next record
    assert 0 < int(long_["name_off"]) < end < chunk < len(text) - 100 and int(tail["seq_len"]) == 3000
    first_with_window = int(np.flatnonzero(recs["n_valid_kmers"] > 0)[0])
    assert first_with_window == 0 and index - first_with_window == s
    without = int(np.count_nonzero(recs["n_valid_kmers"][:s] == 0))
    assert without == (len(range(1, s, 3)) if ragged else 0)
    # bases of the chunk in front of the long record: all of them, or at least those of the reads that have a window
    for before in (int(recs["seq_len"][:s].sum()), int(recs["seq_len"][:s][recs["n_valid_kmers"][:s] > 0].sum())):
        assert (before + 12_000) // 1024 - -(-before // 1024) >= 2
