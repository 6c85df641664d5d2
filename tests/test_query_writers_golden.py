"""CPU: the files of write_kmq / write_kmb / write_kmh / write_kmp, whole.  tests/golden/query_writers.json was recorded by
running this module as a script on the commit before the four writers were folded into one (`python tests/test_query_writers_golden.py`
writes it anew from whatever writers the tree holds): nothing in it was written by hand.  It holds the text of every `.tsv` and
`.json` and, since the members of a zip carry times, every npz entry as dtype, shape and values."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "query_writers.json")
COLUMNS = ["ta", "tb", "tc"]
CASES = ("record", "record_qual", "binned", "binned_coords_qual")


def _u64(rows):
    return np.array(rows, dtype=np.uint64)


def _spectrum(n_windows, seed):
    """(rows, 3, 256): every row's windows spread over a few counts, the same number in every table."""
    spec = np.zeros((len(n_windows), 3, 256), dtype=np.uint64)
    for r, m in enumerate(n_windows):
        for t in range(3):
            for j in range(m):
                spec[r, t, (seed + 7 * r + 3 * t + 5 * j) % 11 * (t + 1)] += np.uint64(1)
    return spec


def fixed_result(case: str) -> dict:
    """3 records, the second without a window, 3 tables, W = 2: rows 0-2 are record 0's bins, rows 3-4 record 2's."""
    from pykmer_amd.qspectrum import median_from_spectrum
    from pykmer_amd.spectrum import pair_list
    res = {"names": ["r0", " r1 \t", "r2 desc"], "seq_len": _u64([13, 4, 11]), "n_valid": _u64([5, 0, 3]),
           "hits": _u64([[5, 2, 0], [0, 0, 0], [1, 3, 2]]), "depth": _u64([[9, 400, 0], [0, 0, 0], [255, 3, 7]]),
           "kmer_len": 9, "min_count": 2, "max_count": 200,
           "spectrum": _spectrum([5, 0, 3], 1), "shared": _u64([[2, 0, 0], [0, 0, 0], [1, 1, 2]]), "pairs": pair_list(3)}
    if case.endswith("qual"):
        res.update(min_qual=20, qual_offset=64)
    if case.startswith("binned"):
        res.update(bin_windows=2, bin_first=_u64([0, 3, 3, 5]),
                   bin_hits=_u64([[2, 1, 0], [2, 1, 0], [1, 0, 0], [1, 2, 1], [0, 1, 1]]),
                   bin_depth=_u64([[4, 200, 0], [4, 200, 0], [1, 0, 0], [255, 2, 3], [0, 1, 4]]),
                   bin_spectrum=_spectrum([2, 2, 1, 2, 1], 2),
                   bin_shared=_u64([[1, 0, 0], [1, 0, 0], [0, 0, 0], [1, 1, 1], [0, 0, 1]]))
        res["bin_median"] = median_from_spectrum(res["bin_spectrum"])          # the per-record case leaves the median to write_kmh
    if "coords" in case:
        res.update(bin_start=_u64([0, 2, 5, 1, 8]), bin_end=_u64([10, 13, 13, 10, 11]))
    return res


def write_all(case: str) -> list:
    """Every writer the case has files for, into the current directory under the project name `proj`."""
    from pykmer_amd import query
    res = fixed_result(case)
    data = [{"pos": i, "index_file": Path(f"t{i}.kin"), "description_file": Path(f"t{i}.kin.json"), "header": {"kmer_len": 9}} for i in range(3)]
    writers = [query.write_kmq, query.write_kmh, query.write_kmp] + ([query.write_kmb] if case.startswith("binned") else [])
    for write in writers:
        write("proj", res, "q.fq" if case.endswith("qual") else "q.fa", data, COLUMNS)
    return sorted(os.listdir("."))


def snapshot(files: list) -> dict:
    out = {}
    for name in files:
        if name.endswith((".tsv", ".json")):
            with open(name) as fh:
                out[name] = fh.read()
        else:
            with np.load(name) as z:
                out[name] = {key: {"dtype": str(z[key].dtype), "shape": list(z[key].shape), "values": z[key].ravel().tolist()} for key in sorted(z.files)}
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("case", CASES)
def test_the_files_are_those_of_the_recorded_writers(case, golden, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    files = write_all(case)
    want = golden[case]
    assert files == sorted(want) and not [f for f in files if f.endswith(".tmp")]
    assert len(files) == (12 if case.startswith("binned") else 9)
    got = snapshot(files)
    for name in files:
        if isinstance(want[name], str):
            assert got[name] == want[name], name
            continue
        assert sorted(got[name]) == sorted(want[name]), name
        for key, entry in want[name].items():
            assert got[name][key] == entry, (name, key)


if __name__ == "__main__":
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    recorded = {}
    for case_ in CASES:
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            recorded[case_] = snapshot(write_all(case_))
            os.chdir("/")
    with open(GOLDEN, "w") as fh:
        json.dump(recorded, fh, sort_keys=True, indent=0)
        fh.write("\n")
