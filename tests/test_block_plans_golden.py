"""The routes of block_sum / block_psum / block_sort, pinned: ek_hip_reduce_blocks_plan, ek_hip_psum_blocks_plan and
ek_hip_sort_blocks_plan reproduce every tuple of tests/golden/block_plans.npz exactly.  Host only, no GPU needed.

The file holds the six numeric types x compute units {0, 1, 256, 304} x 23 block sizes on both sides of every route boundary x 9
block counts on both sides of 2 x #CU.  It was written ONCE (tests/golden/make_block_plans.py), from the library as it stood before
the four block_*.hip files got their shared header csrc/ek_block.h, and is never regenerated from the code under test: a plan that
moves is a change of behaviour that has to be argued for, with a new file, in its own right."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_plans.npz")


@pytest.fixture(scope="module")
def capi():
    from enoki_amd import capi as c        # (loading the library and asking for a plan needs no device)
    return c


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def test_the_grid_is_the_recorded_one(golden):
    grid = golden["grid"]
    assert list(golden["dtypes"]) == ["int32", "uint32", "int64", "uint64", "float32", "float64"]
    assert sorted(set(grid[:, 0].tolist())) == list(range(6)) and sorted(set(grid[:, 1].tolist())) == [0, 1, 256, 304]
    assert sorted(set(grid[:, 2].tolist())) == [1, 2, 3, 5, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 8191, 8192, 8193,
                                                16383, 16384, 16385, 2 ** 20, 2 ** 20 + 4]
    assert sorted(set(grid[:, 3].tolist())) == [1, 2, 3, 511, 512, 513, 607, 608, 609]
    assert len(grid) == 6 * 4 * 23 * 9 and len(np.unique(grid, axis=0)) == len(grid)
    assert golden["reduce"].shape == (len(grid), 3) and golden["psum"].shape == (len(grid), 3) and golden["sort"].shape == (len(grid), 5)
    # the grid reaches every route of the three plans
    assert set(golden["reduce"][:, 0].tolist()) == {0, 1, 2, 3, 4} and set(golden["psum"][:, 0].tolist()) == {0, 1, 2, 3}
    assert set(golden["sort"][:, 0].tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("which", ["reduce", "psum", "sort"])
def test_plans_are_the_recorded_ones(capi, golden, which):
    plan = {"reduce": lambda dt, n, B, cu: capi.reduce_blocks_plan(dt, n, B, cu),
            "psum": lambda dt, n, B, cu: capi.psum_blocks_plan(dt, n, B, cu),
            "sort": lambda dt, n, B, cu: capi.sort_blocks_plan(dt, n, B, True, cu)}[which]
    dtypes = [str(d) for d in golden["dtypes"]]
    got = np.array([plan(dtypes[t], m * B, B, cu) for t, cu, B, m in golden["grid"].tolist()], dtype=np.int64)
    want = golden[which]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, [(dtypes[golden["grid"][i, 0]], *golden["grid"][i, 1:].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:5]]
