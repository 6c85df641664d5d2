"""bench.py at a toy size: a plain run prints the bench line alone, --full adds the merge, CPU and end-to-end legs, and
--dump-outputs writes the same arrays either way."""
import json
import os

import numpy as np
import pytest

from gpu_support import run_py

pytestmark = pytest.mark.gpu
SMALL = ["--bp", "2000000", "--k", "11", "--steps", "2", "--warmup", "1", "--merge-n", "3", "--merge-bp", "1000000",
         "--no-merge32", "--cpu-bp", "1000000"]
FULL_ONLY = {"merge", "merge_n32", "cpu_baseline", "e2e"}


def _bench(*flags, cwd):
    return json.loads(run_py("bench.py", *SMALL, *flags, cwd=cwd).stdout.strip().splitlines()[-1])


def _dump(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_and_full_runs(gpu, tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"), cwd=str(tmp_path))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "stage_ms", "roofline"):
        assert key in plain, key
    assert plain["unit"] == "bp/s" and plain["higher_is_better"] is True and plain["dtype"] == "u8"
    assert not FULL_ONLY & set(plain), sorted(FULL_ONLY & set(plain))
    got = _dump(tmp_path / "plain")
    assert "merge_n3_pairs.npy" in got and "table_sample.npy" in got
    assert int(got["num_kmers.npy"][0]) == plain["config"]["num_kmers"]

    full = _bench("--full", "--dump-outputs", str(tmp_path / "full"), cwd=str(tmp_path))
    for key in ("merge", "cpu_baseline", "e2e"):
        assert "error" not in full[key], full[key]
    assert full["cpu_baseline"]["all_cores"]["table_equals_gpu_table"]
    assert full["merge"]["cpu_baseline"]["slice_equals_gpu"]
    want = _dump(tmp_path / "full")
    assert got.keys() == want.keys()
    for name in got:
        assert np.array_equal(got[name], want[name]), name
