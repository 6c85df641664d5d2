"""GPU: per-record k-mer hits (kmer_query.hip, pk_query_*) against the host restatement (query_ref), exact equality."""
import gzip
import json
import os

import numpy as np
import pytest

import gpu_support as gs
import inputs
import oracle
import query_ref
import synth
from gpu_support import Device, index_cli, lib, query, run_py, same, stream
from host_support import write_kin

pytestmark = pytest.mark.gpu
CHUNK = 16384
WINDOWS = ((1, 255), (2, 254), (255, 255), (1, 1))


# ------------------------------------------------------------------ 1. edge grammar ----------------
@pytest.mark.parametrize("k", [1, 3, 5, 7, 9, 11])
def test_edge_grammar(gpu, k):
    tables = query_ref.random_tables(k, 3, seed=k)
    texts = [inputs.edge_fasta(), inputs.byte_soup(40_000, 11), inputs.byte_soup(40_000, 12)]
    with Device(tables) as dev:
        for text in texts:
            for mn, mx in WINDOWS:
                want = query_ref.expected(text, k, tables, mn, mx)
                same(query(text, k, dev.ptrs, mn, mx), want)
    want = query_ref.expected(texts[0], k, tables, 1, 255)
    assert (want["n_valid"] == 0).any() and want["hits"].any()           # records with no window are listed, others hit


# ------------------------------------------------------------------ 2. slot seams ------------------
@pytest.mark.parametrize("k", [1, 9, 13, 15, 17])
def test_slot_seams(gpu, k):
    if k == 17:
        return _slot_seams_k17()
    text = query_ref.seam_text(k)
    assert len(text) > 6 * CHUNK
    if k <= 9:
        tables = query_ref.random_tables(k, 2, seed=21)
    else:                                                    # 64 MiB / 1 GiB each: cheap to fill, every count-window edge frequent
        pool = np.array([0, 1, 254, 255, 7, 0, 1, 255], dtype=np.uint8)
        tables = [np.tile(np.roll(pool, i), 4 ** k // 8) for i in range(2)]
        tables[1] = np.roll(tables[1], 3)
    with Device(tables) as dev:
        for mn, mx in ((1, 255), (2, 254)):
            same(query(text, k, dev.ptrs, mn, mx), query_ref.expected(text, k, tables, mn, mx))


def _slot_seams_k17():
    """k = 17: the window history is all 16 bases in front of a thread's own, so the chunk start state decides the first
    windows of every slot.  The table is counted on the GPU from stretches of the seam text around every chunk boundary:
    windows across the boundaries without an N hit, and so do the windows next to the two seams.  Feeds cut 3 bytes before
    and behind the seams' chunk boundaries give the same result."""
    lib = gs.lib()
    k = 17
    text = query_ref.seam_text(k)
    counted = query_ref.counted_text_for(text, k, seed=1700)
    sparse = [query_ref.SparseTable(oracle.kmer_list(counted, k))]
    kmers = oracle.kmer_list(text, k)
    start, straddles, first_base = query_ref.straddling_windows(text, k)
    assert start.size == kmers.size
    count = sparse[0][kmers]
    across = {b: count[straddles == b] for b in range(CHUNK, len(text), CHUNK)}
    for b, c in across.items():                              # no valid window lies across a seam; k - 1 lie across any other boundary
        assert c.size == (0 if b in (2 * CHUNK, 5 * CHUNK) else k - 1), b
    assert all((across[b] == 1).all() for b in (CHUNK, 3 * CHUNK)) and all((across[b] == 2).all() for b in (4 * CHUNK, 6 * CHUNK))
    for b in (2 * CHUNK, 5 * CHUNK):                         # the nearest windows on either side of a seam hit
        i = int(np.searchsorted(start, first_base[b])) - 1
        assert start[i] + k <= first_base[b] < start[i + 1] and count[i] >= 1 and count[i + 1] >= 1, b
    assert 0 < np.count_nonzero(count) < count.size // 10
    with lib.Indexer(k, device=0) as ix:
        ix.feed(counted)
        ix.finish()
        ptrs = [ix.table_device_ptr()]
        for mn, mx in ((1, 255), (2, 254)):
            want = query_ref.expected(text, k, sparse, mn, mx)
            assert want["hits"][0, 0] > 0
            whole = query(text, k, ptrs, mn, mx)
            same(whole, want)
            for sign in (-3, 3):
                cut = query(text, k, ptrs, mn, mx, cuts=[2 * CHUNK + sign, 5 * CHUNK + sign])
                assert np.array_equal(cut["hits"], whole["hits"]) and np.array_equal(cut["depth"], whole["depth"]), sign
                assert np.array_equal(cut["records"], whole["records"])


# ------------------------------------------------------------------ 2b. a long record late in a slot
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("s", [126, 127, 128, 129, 200])
def test_long_record_behind_short_ones(gpu, s, ragged):
    """A record of 12 000 bases as record s of its slot: whole waves of it are summed across the wave and added by one lane,
    to the slot's LDS tallies below index 128 and to HBM from there on (tests/test_query_host.py checks the layout)."""
    k = 9
    text, index = query_ref.long_after_short(s, seed=300 + s, ragged=ragged)
    tables = query_ref.random_tables(k, 2, seed=22)
    with Device(tables) as dev:
        for mn, mx in ((1, 255), (2, 254)):
            want = query_ref.expected(text, k, tables, mn, mx)
            assert want["n_valid"][index] == 12_000 - k + 1 and want["hits"][index].all()
            same(query(text, k, dev.ptrs, mn, mx), want)


# ------------------------------------------------------------------ 3. many records ----------------
def test_many_records_per_piece_and_chunk(gpu):
    k = 9
    text = query_ref.reads_text(k)
    tables = query_ref.random_tables(k, 2, seed=32)
    want = query_ref.expected(text, k, tables, 1, 254)
    assert len(want["records"]) == 6000 > 4096               # beyond the record array's first capacity: the squeeze backs out once
    with Device(tables) as dev:
        got = query(text, k, dev.ptrs, 1, 254)
    same(got, want)
    empty = want["n_valid"] == 0
    assert empty.sum() > 1000 and got["hits"].shape[0] == 6000 and not got["hits"][empty].any() and not got["depth"][empty].any()


# ------------------------------------------------------------------ 4. feeds -----------------------
def test_feeds_cut_anywhere_and_reset(gpu):
    k = 9
    reads, seams = query_ref.reads_text(k), query_ref.seam_text(k)
    tables = query_ref.random_tables(k, 2, seed=41)
    with Device(tables) as dev:
        for text in (reads, seams):
            whole = query(text, k, dev.ptrs, 2, 255)
            same(whole, query_ref.expected(text, k, tables, 2, 255))
            at = text.find(b">", 3 * CHUNK + 100)
            hdr = at + 2 if at >= 0 else 3 * CHUNK + 100     # inside a header (reads); the one-record text has none there
            cuts = sorted({7, 8, CHUNK, CHUNK + 5, 2 * CHUNK - 3, 3 * CHUNK, hdr, 4 * CHUNK + 61 * 3 + 4, len(text) - 1})
            cut = query(text, k, dev.ptrs, 2, 255, cuts=cuts)   # 7..8: one byte; CHUNK, 3 * CHUNK: ends at a chunk multiple; the rest inside k-mers
            for key in ("hits", "depth"):
                assert np.array_equal(cut[key], whole[key]), key
            assert np.array_equal(cut["records"], whole["records"])
        # a second stream after reset: its own results, nothing carried over
        with lib().QueryIndexer(k, device=0) as q:
            q.set_tables(dev.ptrs, 2, 255)
            r = reads[:5000].count(b">")
            assert 3 * r + 1024 <= 4096 < reads.count(b">")                # the record array grows in the second feed, over the first feed's rows
            first = stream(q, reads, cuts=[5000])
            second = stream(q, seams, cuts=[CHUNK + 1])
            q.set_tables(dev.ptrs[:1], 1, 1)                  # and other tables / another window after a reset
            third = stream(q, reads)
        assert not any(got["fin"]["hist256"].any() for got in (first, second, third))
        same(first, query_ref.expected(reads, k, tables, 2, 255))
        same(second, query_ref.expected(seams, k, tables, 2, 255))
        same(third, query_ref.expected(reads, k, tables[:1], 1, 1))


# ------------------------------------------------------------------ 5. FASTQ -----------------------
def test_fastq_reads(gpu):
    k = 9
    rng = np.random.default_rng(51)
    out = []
    for i in range(3000):
        n = int(rng.integers(30, 151))
        seq = np.frombuffer(b"ACGTACGTACGTN", dtype=np.uint8)[rng.integers(0, 13, n)].tobytes()
        out.append(b"@read%d extra\r\n" % i + seq + b"\r\n+\r\n" + bytes(rng.integers(33, 74, n, dtype=np.uint8)) + b"\r\n")
    fq = b"".join(out)
    tables = query_ref.random_tables(k, 2, seed=52)
    want = query_ref.expected(fq, k, tables, 1, 255, fmt="fastq")
    assert len(want["records"]) == 3000
    with Device(tables) as dev:
        same(query(fq, k, dev.ptrs, fmt="fastq"), want)
        same(query(fq, k, dev.ptrs, fmt="fastq", cuts=[1, 100_003, 2 * CHUNK]), want)


# ------------------------------------------------------------------ 6. full-size tables ------------
@pytest.mark.parametrize("k,n_tables", [(15, 2), (17, 1)])
def test_full_size_tables_counted_on_the_gpu(gpu, k, n_tables):
    """32-bit (k = 15) and 64-bit (k = 17) k-mers against tables that were counted on the GPU and never left HBM."""
    lib = gs.lib()
    genomes = [synth.family(i, 200_000)[0] for i in range(n_tables + 1)]
    text = bytes(genomes[n_tables]) + bytes(genomes[0])      # another family member, then one of the indexed genomes itself
    sparse = [query_ref.SparseTable(oracle.kmer_list(g, k)) for g in genomes[:n_tables]]
    indexers = []
    try:
        for g in genomes[:n_tables]:
            ix = lib.Indexer(k, device=0)
            indexers.append(ix)
            ix.feed(g)
            ix.finish()
        ptrs = [ix.table_device_ptr() for ix in indexers]
        for mn, mx in ((1, 255), (2, 255)):
            want = query_ref.expected(text, k, sparse, mn, mx)
            got = query(text, k, ptrs, mn, mx)
            same(got, want)
            if (mn, mx) == (1, 255):
                n_self = len(oracle.kmer_list(genomes[0], k, records=True)[1]["records"])
                assert n_self >= 1 and np.array_equal(got["hits"][-n_self:, 0], want["n_valid"][-n_self:])
                assert 0 < got["hits"][:-n_self, 0].sum() < want["n_valid"][:-n_self].sum()
    finally:
        for ix in indexers:
            ix.close()


# ------------------------------------------------------------------ 7. table counts ----------------
def test_table_counts_and_the_group_loop(gpu):
    """N = 1, 13 and 17 (one launch takes 16 tables, so 17 runs the group loop): column t equals the 1-table run on table t."""
    k = 9
    text = query_ref.reads_text(k, n_reads=1500, seed=71) + inputs.byte_soup(30_000, 72)
    tables = query_ref.random_tables(k, 17, seed=73)
    with Device(tables) as dev:
        single = [query(text, k, dev.ptrs[t:t + 1], 1, 254) for t in range(17)]
        same(single[0], query_ref.expected(text, k, tables[:1], 1, 254))
        for n in (13, 17):
            got = query(text, k, dev.ptrs[:n], 1, 254)
            assert got["hits"].shape[1] == n
            for t in range(n):
                assert np.array_equal(got["hits"][:, t], single[t]["hits"][:, 0]), (n, t)
                assert np.array_equal(got["depth"][:, t], single[t]["depth"][:, 0]), (n, t)
        same(got, query_ref.expected(text, k, tables, 1, 254))


# ------------------------------------------------------------------ 7b. file-backed table groups --
def test_file_backed_tables_staged_group_after_group(gpu, tmp_path):
    """query_records on real files with a budget of two tables: five tables (one of them BGZF) are staged from their files
    in three groups, the query is streamed once per group, and every byte of a raw table is read exactly once."""
    from pykmer_amd import bgzf, query
    from pykmer_amd.header import Header
    k, N = 9, 5
    paths, tables, bases = [], [], []
    for i in range(N):
        fa, _ = synth.family(i, 60_000)
        w = write_kin(tmp_path, f"q{i}.fa", fa.tobytes(), k)
        paths.append(w.path)
        tables.append(w.table)
        bases.append(b"".join(ln for ln in fa.tobytes().split(b"\n") if not ln.startswith(b">")))
    bgzf.compress_file(paths[2], level=1)
    headers = [Header(p, index_file=p) for p in paths]
    assert headers[2].index_file.endswith(".bgz")
    text = b"".join(b">r%d of sample %d\n" % (i, i % N) + bases[i % N][700 * i:700 * i + 250 + 37 * i] + b"\n" for i in range(6))
    qf = tmp_path / "q.fa"
    qf.write_bytes(text)
    got = query.query_records(str(qf), headers, 2, 254, device=0, hbm_budget=2 * 4 ** k + 100)
    assert got["n_groups"] == 3
    want = query_ref.expected(text, k, tables, 2, 254)
    assert len(got["names"]) == 6 and got["hits"].shape == (6, N) and want["hits"].any(axis=0).all()
    assert np.array_equal(got["n_valid"], want["n_valid"]) and np.array_equal(got["seq_len"], want["seq_len"])
    assert np.array_equal(got["hits"], want["hits"]), np.argwhere(got["hits"] != want["hits"])[:5]
    assert np.array_equal(got["depth"], want["depth"]), np.argwhere(got["depth"] != want["depth"])[:5]
    assert all(h.bytes_delivered == 4 ** k for i, h in enumerate(headers) if i != 2)


# ------------------------------------------------------------------ 8. CLI -------------------------
def test_cli_end_to_end(gpu, tmp_path):
    k = 9
    kins, tables = index_cli(tmp_path, ("s0", "s1", "s2"), k)
    with open(kins[1], "rb") as fh:
        raw = fh.read()
    with gzip.open(kins[1] + ".bgz", "wb") as out:
        out.write(raw)
    os.remove(kins[1])
    kins[1] += ".bgz"
    text = query_ref.reads_text(k, n_reads=800, seed=81) + bytes(synth.family(1, 20_000)[0])
    qf = tmp_path / "queries.fa.gz"
    with gzip.open(qf, "wb") as out:
        out.write(text)
    want = query_ref.expected(text, k, tables, 2, 250)
    names = [n.strip() for n in query_ref.names(text, want["records"])]

    def check(proj):
        z = np.load(proj + ".kmq")
        for key in ("hits", "depth", "n_valid", "seq_len"):
            assert z[key].dtype == np.uint64 and np.array_equal(z[key], want[key]), key
        assert (int(z["kmer_len"]), int(z["min_count"]), int(z["max_count"])) == (k, 2, 250)
        with open(proj + ".kmq.json") as fh:
            meta = json.load(fh)
        assert meta["records"] == names and meta["kmer_len"] == k and meta["query_file"] == str(qf)
        assert [os.path.basename(d["index_file"]) for d in meta["data"]] == [os.path.basename(p) for p in kins]
        lines = open(proj + ".kmq.tsv").read().split("\n")
        assert lines[0].split("\t")[:3] == ["record", "seq_len", "n_valid"] and len(lines[0].split("\t")) == 6
        rows = [ln.split("\t") for ln in lines[1:-1]]
        assert [r[0] for r in rows] == names
        assert np.array_equal(np.array([[int(v) for v in r[3:]] for r in rows], dtype=np.uint64), want["hits"])
        return [open(proj + ext, "rb").read() for ext in (".kmq", ".kmq.json", ".kmq.tsv")]

    a = str(tmp_path / "proj")
    run_py("query.py", a, str(qf), *kins, "--min-count", "2", "--max-count", "250", cwd=str(tmp_path))
    files_a = check(a)
    b = str(tmp_path / "grouped")
    out = run_py("query.py", b, str(qf), *kins, "--min-count", "2", "--max-count", "250", cwd=str(tmp_path),
                 env=dict(os.environ, PK_MERGE_HBM_BUDGET=str(2 * 4 ** k + 1000))).stdout
    assert "2 table group(s)" in out
    files_b = check(b)
    assert files_a[0] == files_b[0] and files_a[2] == files_b[2]
    assert json.loads(files_a[1].replace(a.encode(), b"P")) == json.loads(files_b[1].replace(b.encode(), b"P"))


# ------------------------------------------------------------------ 9. state errors ----------------
def test_state_errors(gpu):
    lib = gs.lib()
    k = 9
    tables = query_ref.random_tables(k, 1, seed=91)
    text = inputs.edge_fasta()
    with Device(tables) as dev, lib.QueryIndexer(k, device=0) as q:
        with pytest.raises(lib.PkError) as e:
            q.feed(text)                                     # no tables yet
        assert e.value.code == lib.PK_ERR_STATE
        q.reset()
        q.set_tables(dev.ptrs, 1, 255)
        q.feed(text)
        with pytest.raises(lib.PkError) as e:
            q.set_tables(dev.ptrs, 1, 255)
        assert e.value.code == lib.PK_ERR_STATE
        with pytest.raises(lib.PkError) as e:
            q.results(10)                                    # before finish
        assert e.value.code == lib.PK_ERR_STATE
        fin = q.finish()
        assert fin["n_records"] > 2
        for call in (q.table_to_host, q.table_device_ptr):
            with pytest.raises(lib.PkError) as e:
                call()
            assert e.value.code == lib.PK_ERR_STATE
        with pytest.raises(lib.PkError) as e:
            q.results(fin["n_records"] - 1)
        assert e.value.code == lib.PK_ERR_RECS_CAP
        hits, _ = q.results(fin["n_records"])
        assert np.array_equal(hits, query_ref.expected(text, k, tables, 1, 255)["hits"])
    for bad_k in (8, 19, 0):
        with pytest.raises(ValueError):
            lib.QueryIndexer(bad_k, device=0)
    with lib.Indexer(k, device=0) as ix:                     # a counting indexer takes no tables
        with pytest.raises(lib.PkError) as e:
            lib._check(lib.load().pk_query_set_tables(ix._h, None, 1, 1, 255))
        assert e.value.code == lib.PK_ERR_STATE
