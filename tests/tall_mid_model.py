"""TEST INFRASTRUCTURE: the batched tall mid-size SVD (m > 128, 65 to 128
columns; brd_qr_mid_batched.hip around brd_svd_mid_batched.hip; DESIGN.md
"Batched tall mid-size SVD") in terms of the existing models.

The method is tests/tall_model.py's at the row-block height of the 128-column
class: tall_qr(A, dt, rb=RB), jacobi_model.jacobi_svd on R, apply_q.  The
checks and limits are tests/mid_model.py's (jacobi_model.LIMITS x n / 64).
This file only fixes RB and the shapes the model test and the GPU test share.
"""
from __future__ import annotations

import numpy as np

from tall_model import tall_svd

RB = 128             # rows per block of the 128-column class
FORWARD_ROWS = 128   # at most this many rows: the Jacobi kernels as they are


def tall_mid_svd(A, dtype=None):
    """(U, S, V, info) by the QR front end at RB rows per block."""
    return tall_svd(A, dtype=dtype, rb=RB)


def gpu_shapes():
    """n in {65, 96, 127, 128} (the smallest and largest column counts of the
    class) with 129, RB, RB + 1, RB + n, RB + n + 1 and 2 RB + n + 1 rows where
    that is more than 128 rows (the first-block boundary, one row into the
    second block, a ragged last block), plus 1000 x 72 and 2049 x 128."""
    shapes = []
    for n in (65, 96, 127, 128):
        for m in (129, RB, RB + 1, RB + n, RB + n + 1, 2 * RB + n + 1):
            if m > FORWARD_ROWS and m >= n and (m, n) not in shapes:
                shapes.append((m, n))
    return shapes + [(1000, 72), (2049, 128)]


GPU_SHAPES = gpu_shapes()


def uniform_batch(m, n, count=3):
    """uniform(0, 5) inputs by the seed rule of tests/test_gpu_svd_batched.py."""
    return np.random.default_rng(1000 * m + n).uniform(0, 5, (count, m, n))
