"""Writes block_plans.npz: what ek_hip_reduce_blocks_plan, ek_hip_psum_blocks_plan and ek_hip_sort_blocks_plan report over a grid of
(type, compute units, block, blocks).  Host only.

The committed file was written ONCE, from the library as it stood before the block primitives got their shared header
(csrc/ek_block.h), and pins the plans from then on.  It is not to be regenerated from the code that
tests/test_block_plans_golden.py checks: run this only against a library whose plans are known to be the wanted ones.

    python tests/golden/make_block_plans.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

DTYPES = ["int32", "uint32", "int64", "uint64", "float32", "float64"]
CUS = [0, 1, 256, 304]
BLOCKS = [1, 2, 3, 5, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 2 ** 20, 2 ** 20 + 4]
COUNTS = [1, 2, 3, 511, 512, 513, 607, 608, 609]      # m = n / B: both sides of 2 x cu for 256 and 304 compute units


def grid():
    """rows (type, compute units, B, m), in a fixed order"""
    return np.array([(t, cu, B, m) for t in range(len(DTYPES)) for cu in CUS for B in BLOCKS for m in COUNTS], dtype=np.int64)


def plans(capi, rows):
    """per row: reduce (regime, splits, workgroups), psum (regime, splits, workgroups), sort (route, tile_rows, chunk, passes, workgroups)"""
    red, scan, sort = [], [], []
    for t, cu, B, m in rows.tolist():
        red.append(capi.reduce_blocks_plan(DTYPES[t], m * B, B, cu))
        scan.append(capi.psum_blocks_plan(DTYPES[t], m * B, B, cu))
        sort.append(capi.sort_blocks_plan(DTYPES[t], m * B, B, True, cu))
    return np.array(red, dtype=np.int64), np.array(scan, dtype=np.int64), np.array(sort, dtype=np.int64)


if __name__ == "__main__":
    from enoki_amd import capi
    rows = grid()
    red, scan, sort = plans(capi, rows)
    np.savez_compressed(os.path.join(HERE, "block_plans.npz"), dtypes=np.array(DTYPES), grid=rows, reduce=red, psum=scan, sort=sort)
    print(f"block_plans.npz: {len(rows)} rows")
