"""The files this build writes, read the way the reference's own Header and merger read them: the name parsed into
input and k (tools.py:220-238), the JSON looked up key by key with the fixed keys checked (tools.py:387-401), the
raw table compared pair-wise (tools.py:439-493).  Every expected value is one the reference itself wrote
(tests/golden/manifest.json), and none of this package's readers is used."""
import json
import os

import numpy as np

from host_support import family_indexes


def _parse_index_name(path):
    """<input>.<kk>.kin: the input's name and k."""
    stem, kk, ext = path.rsplit(".", 2)
    assert ext == "kin" and len(kk) == 2
    return os.path.basename(stem), int(kk)


def test_reference_reads_our_kin_and_merges_it(tmp_path, manifest):
    written = manifest["indexer"]["G3_edge_k7"]                         # a k = 7 .kin.json the reference wrote
    paths = sorted(family_indexes(tmp_path, manifest, n=3))
    tables = []
    for i, path in enumerate(paths):
        assert _parse_index_name(path) == (f"s{i:02d}.fa", 7)
        with open(path + ".json") as fh:
            meta = json.load(fh)
        assert sorted(meta) == written["reference_keys"]
        for f in ("file_ver", "kmer_size", "data_size", "max_size"):
            assert meta[f] == written["expect"][f], f
        assert meta["kmer_len"] == 7
        table = np.fromfile(path, dtype=np.uint8)
        assert table.size == meta["data_size"]
        tables.append(table)
    s_valid, o_valid = ((t >= 2) & (t <= 255) for t in tables[:2])    # min_count=2, as the golden merge ran
    got = (int(s_valid.sum()), int(o_valid.sum()), int((s_valid & o_valid).sum()))
    assert got == tuple(manifest["merger"]["G7_k7_n13_min2"]["matrix"][0][1])
