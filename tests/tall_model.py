"""TEST INFRASTRUCTURE: numpy model of the batched tall SVD
(brd_qr_batched.hip around brd_svd_batched.hip; DESIGN.md "Batched tall SVD").

Not the product path -- it is the executable specification of the front end:
Householder QR of the first row block, every further block B_k folded in as
the QR of the stacked [R; B_k] (reflectors [e_j; v_j]: step j touches row j of
R and the block only), the same row-block height per column class, the same
running power-of-two scale, then jacobi_model.jacobi_svd on R and the blocks'
reflectors applied in reverse order to [U_R; 0].  It works in any numpy float
dtype and is itself checked against numpy.linalg.svd (tests/test_tall_model.py).

Only the order of the floating-point sums differs from the kernels (numpy's
pairwise sum against the kernels' strided loop and shuffle tree).
"""
from __future__ import annotations

import numpy as np

from jacobi_model import jacobi_svd

FORWARD_ROWS = 128   # matrices of at most this many rows go to the Jacobi kernel as they are


def row_block(n: int) -> int:
    """Rows per block of the column class of n (16 / 32 / 64 columns)."""
    return 256 if n <= 32 else 128


def _emax(dt) -> int:
    return -int(np.finfo(dt).minexp)   # 1022 / 126: the kernels' clamp


def _reflector(alpha, x, dt):
    """LAPACK xLARFG on [alpha; x]: (beta, tau, scal) with v = scal * x."""
    s2 = np.sum(x * x)
    if s2 == 0:
        return alpha, dt.type(0), dt.type(0)
    beta = -np.copysign(np.sqrt(alpha * alpha + s2), alpha)
    return beta, (beta - alpha) / beta, dt.type(1) / (alpha - beta)


def tall_qr(A, dtype=None, rb: int | None = None):
    """Blocked Householder QR of the m x n matrix A (m >= n) in ``dtype``.

    Returns (R, blocks): R n x n upper triangular with the scale undone (all
    NaN for a non-finite A); blocks[k] = (row0, V_k, tau_k) with V_k in explicit
    form (first block: zeros above the diagonal and one on it; later blocks:
    the part of [e_j; v_j] below e_j)."""
    dt = np.dtype(dtype if dtype is not None else np.asarray(A).dtype)
    A = np.asarray(A, dtype=dt)
    m, n = A.shape
    assert m >= n >= 1
    rb = rb or row_block(n)
    assert rb >= n
    emax = _emax(dt)
    e = -emax
    R = np.zeros((n, n), dtype=dt)
    blocks = []
    bad = not np.all(np.isfinite(A))
    for row0 in range(0, m, rb):
        B = np.array(A[row0:row0 + rb], dtype=dt, copy=True)
        first = row0 == 0
        fin = np.abs(B[np.isfinite(B)])
        mx = fin.max() if fin.size else 0
        if mx > 0:
            ek = int(np.clip(np.frexp(mx)[1], -emax, emax))
            if ek > e:
                R = np.ldexp(R, e - ek).astype(dt)
                e = ek
        with np.errstate(all="ignore"):
            B = (B * np.ldexp(dt.type(1), -e)).astype(dt)
            tau = np.zeros(n, dtype=dt)
            for j in range(n):
                lo = j + 1 if first else 0
                x = B[lo:, j].copy()
                alpha = B[j, j] if first else R[j, j]
                beta, tau[j], scal = _reflector(alpha, x, dt)
                if j + 1 < n:
                    top = B[j, j + 1:] if first else R[j, j + 1:]
                    w = top + scal * (x @ B[lo:, j + 1:])
                    tw = tau[j] * w
                    top -= tw            # a view: row j of the block or of R
                    B[lo:, j + 1:] -= np.outer(x, tw * scal)
                B[lo:, j] = x * scal
                if first:
                    R[j, j:] = B[j, j:]
                    B[:j, j] = 0
                    B[j, j] = 1
                R[j, j] = beta
        blocks.append((row0, B, tau))
    R = np.triu(np.ldexp(R, e)).astype(dt)
    if bad:
        R[:] = np.nan
    return R, blocks


def apply_q(blocks, UR, m):
    """U = Q [U_R; 0]: the blocks' reflectors in reverse order."""
    dt = UR.dtype
    n = UR.shape[0]
    U = np.zeros((m, n), dtype=dt)
    W = np.array(UR, copy=True)
    for row0, V, tau in reversed(blocks):
        first = row0 == 0
        Cb = np.zeros((V.shape[0], n), dtype=dt)
        if first:
            Cb[:n] = W
        for j in range(n - 1, -1, -1):
            w = V[:, j] @ Cb
            if not first:
                w = w + W[j]
                W[j] -= tau[j] * w
            Cb -= np.outer(V[:, j], tau[j] * w)
        U[row0:row0 + V.shape[0]] = Cb
    return U


def tall_svd(A, dtype=None, rb: int | None = None):
    """(U, S, V, info) like jacobi_model.jacobi_svd, through the QR front end;
    at most FORWARD_ROWS rows: the Jacobi model directly, as the library does."""
    dt = np.dtype(dtype if dtype is not None else np.asarray(A).dtype)
    A = np.asarray(A, dtype=dt)
    m, n = A.shape
    if m <= FORWARD_ROWS:
        return jacobi_svd(A, dtype=dt)[:4]
    R, blocks = tall_qr(A, dt, rb)
    UR, S, V, info, _ = jacobi_svd(R, dtype=dt)
    if info == 2:
        return np.full((m, n), np.nan, dtype=dt), S, V, info
    return apply_q(blocks, UR, m), S, V, info


# ---------------------------------------------------------------------------
# the shapes shared by the model tests and the GPU tests
# ---------------------------------------------------------------------------
BASE_SHAPES = [(129, 1), (129, 64), (130, 3), (192, 64), (193, 64), (256, 16), (257, 33), (300, 64), (513, 17),
               (1000, 64), (4097, 16)]


def gpu_shapes():
    """BASE_SHAPES plus, for every row-block height RB used at a tested n: RB,
    RB + 1, RB + n, RB + n + 1 and 2 RB + n + 1 rows (the first block boundary,
    one row into the second block, a ragged third block)."""
    shapes = list(BASE_SHAPES)
    for n in sorted({n for _, n in BASE_SHAPES}):
        rb = row_block(n)
        for m in (rb, rb + 1, rb + n, rb + n + 1, 2 * rb + n + 1):
            if (m, n) not in shapes:
                shapes.append((m, n))
    return shapes


GPU_SHAPES = gpu_shapes()


def uniform_batch(m, n, count=3):
    """uniform(0, 5) inputs by the seed rule of tests/test_gpu_svd_batched.py."""
    return np.random.default_rng(1000 * m + n).uniform(0, 5, (count, m, n))
