"""CPU: the multi-GPU merge path with world_size=2 over gloo.  Each rank tallies only its slice of the
k-mer address range, the N x N partials are summed by one all-reduce, rank 0 writes the .kma.  The
slice tallies come from the oracle here (no GPU in this suite); on GPUs the same code path calls
pk_gram_device_partial and the all-reduce runs over RCCL."""
import numpy as np
import pytest

from host_support import family_indexes, gloo_merge
from merge_ref import oracle_partial


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_merge_matches_reference_matrix(tmp_path, manifest, world):
    case = manifest["merger"]["G7_k7_n13_min2"]
    paths = sorted(family_indexes(tmp_path, manifest))
    gloo_merge(world, tmp_path, paths, oracle_partial, save_matrix=True, min_count=2, max_count=255)
    want = np.array(case["matrix"], dtype=np.uint64)
    slices = []
    for r in range(world):
        assert np.array_equal(np.load(tmp_path / f"matrix_rank{r}.npy"), want)       # every rank holds the reduced matrix
        lo, hi, delivered = (int(v) for v in np.load(tmp_path / f"slice_rank{r}.npy")[0])
        slices.append((lo, hi))
        # each rank read only its share of every table: N * 4^k / world bytes (+ rounding to 32 addresses)
        assert delivered == len(paths) * (hi - lo) <= len(paths) * (4 ** 7 // world + 32)
    assert slices[0][0] == 0 and slices[-1][1] == 4 ** 7                             # disjoint cover of the address range
    assert all(a[1] == b[0] for a, b in zip(slices[:-1], slices[1:]))
    kma = np.load(tmp_path / "dist.002-255.kma")["matrix"]                           # written once, by rank 0
    assert np.array_equal(kma, want)
