"""TEST INFRASTRUCTURE: numpy model of the batched least squares
(brd_gelss_batched_*; DESIGN.md "Batched least squares").

Not the product path -- it is the executable specification of the whole route
in working precision: the SVD of the route the library picks (jacobi_model /
tall_model / tall_mid_model, by size, as brd_gesvd_batched_* does), then the
three phases of brd_gelss_batched.hip with the same cutoff rule:

    C = L^T B;   C_j *= sigma+_j,  sigma+_j = 1 / sigma_j if sigma_j > rcond sigma_1 else 0;   X = R C

with (L, R) = (U, V) for min |A x - b| and (V, U) for the minimum-norm solution
of A^T x = b (how a wide A is posed).  Only the order of the floating-point
sums differs from the kernel.

It also holds what the model test and the GPU test share: the shapes, the
input generators and the limit functions.  Every limit is built from
mid_model.mid_limits(n, dtype) = (values, reconstruction, orthogonality), the
limits the project puts on the SVD factors themselves: with tol = lim[1] +
lim[2], factors that reconstruct A to lim[1] and are orthogonal to lim[2] give
an x that solves exactly a problem within tol of the one posed.
"""
from __future__ import annotations

import numpy as np

from jacobi_model import jacobi_svd
from mid_model import mid_limits
from tall_model import tall_svd

DT = {"f64": np.float64, "f32": np.float32}

# ---------------------------------------------------------------------------
# shapes: (m, n, right-hand sides).  One per SVD route plus the edges of the
# 16-wide tiles; every shape at nrhs = 1 and one other value, every nrhs value
# at one n <= 64 and one n > 64.
# ---------------------------------------------------------------------------
LS_SHAPES = [(5, 3, 1), (5, 3, 2), (64, 64, 1), (64, 64, 16), (128, 64, 1), (128, 64, 17), (300, 33, 1),
             (300, 33, 33), (128, 96, 1), (128, 96, 2), (128, 128, 1), (128, 128, 16), (129, 65, 1), (129, 65, 17),
             (300, 72, 1), (300, 72, 33), (257, 128, 1), (257, 128, 17)]
WIDE_SHAPES = [(72, 400, 1), (72, 400, 17), (3, 5, 1), (3, 5, 2)]      # solved through the transpose
PINV_SHAPES = [(128, 128), (300, 72), (72, 400)]
DEFICIENT = [(300, 72, 40), (200, 100, 60), (40, 16, 9)]                # (m, n, rank)
DEFICIENT_RCOND = {np.float64: 1e-10, np.float32: 1e-4}
DEFICIENT_NRHS = 3


def uniform_system(m, n, nrhs, count=3):
    """A uniform(0, 5) by the seed rule of tests/test_gpu_svd_batched.py, B uniform(-1, 1)."""
    rng = np.random.default_rng(1000 * m + n)
    A = rng.uniform(0, 5, (count, m, n))
    B = np.random.default_rng(77000 + 1000 * m + 10 * n + nrhs).uniform(-1, 1, (count, m, nrhs))
    return A, B


def deficient_system(m, n, r, count=3):
    """A = G1 G2 with inner dimension r (standard normal factors), B uniform(-1, 1)."""
    rng = np.random.default_rng(500000 + 1000 * m + n)
    A = rng.standard_normal((count, m, r)) @ rng.standard_normal((count, r, n))
    return A, rng.uniform(-1, 1, (count, m, DEFICIENT_NRHS))


def default_rcond(m, n, dtype):
    return max(m, n) * float(np.finfo(dtype).eps)


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def route_svd(A, dtype):
    """(U, S, V, info) of a tall A by the route brd_gesvd_batched_* takes."""
    m, n = A.shape
    assert m >= n
    if m <= 128:
        return jacobi_svd(A, dtype=dtype)[:4]
    return tall_svd(A, dtype=dtype, rb=128 if n > 64 else None)


def solve_phases(L, R, S, B, rcond):
    """The kernel's three phases in the dtype of the factors.  B None: the identity."""
    dt = S.dtype
    C = L.T.copy() if B is None else (L.T @ np.asarray(B, dtype=dt)).astype(dt)
    keep = S > dt.type(rcond) * S[0]
    with np.errstate(divide="ignore"):
        inv = np.where(keep, dt.type(1) / S, dt.type(0)).astype(dt)
    C = (C * inv[:, None]).astype(dt)
    return (R @ C).astype(dt), int(np.count_nonzero(keep))


def model_lstsq(A, B, rcond=None, dtype=np.float64):
    """(X, rank, S) for one matrix A (any orientation) and B (rows of A x nrhs,
    or None for the pseudo-inverse), everything in ``dtype``."""
    dt = np.dtype(dtype)
    A = np.asarray(A, dtype=dt)
    m, n = A.shape
    rc = default_rcond(m, n, dt) if rcond is None else rcond
    if m >= n:
        U, S, V, info = route_svd(A, dt)
        L, R = U, V
    else:
        U, S, V, info = route_svd(np.ascontiguousarray(A.T), dt)
        L, R = V, U
    if info == 2:
        k = m if B is None else np.asarray(B).shape[1]
        return np.full((n, k), np.nan, dtype=dt), -1, S
    X, rank = solve_phases(L, R, S, B, rc)
    return X, rank, S


# ---------------------------------------------------------------------------
# limits (float64 arithmetic on the input rounded to the dtype under test)
# ---------------------------------------------------------------------------
def tol_of(n, dtype):
    """lim[1] + lim[2] at n columns (n: the smaller dimension of A)."""
    lim = mid_limits(n, dtype)
    return lim[1] + lim[2]


def backward_errors(A64, X, B64):
    """Per right-hand side: |A^T (b - A x)|_2 / (|A|_F^2 |x|_2 + |A|_F |b|_2)."""
    X = np.asarray(X, dtype=np.float64)
    na = np.linalg.norm(A64)
    num = np.linalg.norm(A64.T @ (B64 - A64 @ X), axis=0)
    den = na * na * np.linalg.norm(X, axis=0) + na * np.linalg.norm(B64, axis=0)
    return num / den


def forward_fractions(A64, X, B64, Xref, tol, kappa=None, sv=None):
    """Per right-hand side |x - x_ref|_2 over Wedin's bound with perturbation
    size tol: tol kappa (1 + kappa |r| / (|A|_2 |x|)) |x|, kappa and r = b - A
    x_ref from the float64 reference (kappa None: sigma_1 / sigma_min)."""
    X = np.asarray(X, dtype=np.float64)
    sv = np.linalg.svd(A64, compute_uv=False) if sv is None else sv
    kappa = sv[0] / sv[-1] if kappa is None else kappa
    nx = np.linalg.norm(Xref, axis=0)
    nr = np.linalg.norm(B64 - A64 @ Xref, axis=0)
    bound = tol * kappa * (1 + kappa * nr / (sv[0] * nx)) * nx
    return np.linalg.norm(X - Xref, axis=0) / bound


def penrose_fractions(A64, P, tol):
    """The four Penrose conditions as fractions of tol, each relative to c =
    |A|_F |P|_F times the norm of what it compares: A P A = A (c |A|_F), P A P
    = P (c |P|_F), A P and P A symmetric (c: they are products of norm <= c).
    c >= kappa: the factors' loss of orthogonality, lim[2], enters A P = U S
    (V^T V) S+ U^T as S (V^T V - I) S+, whose entries are scaled by up to
    sigma_1 / sigma_n."""
    P = np.asarray(P, dtype=np.float64)
    na, npn = np.linalg.norm(A64), np.linalg.norm(P)
    c = na * npn
    AP, PA = A64 @ P, P @ A64
    return np.array([np.linalg.norm(AP @ A64 - A64) / (c * na), np.linalg.norm(PA @ P - P) / (c * npn),
                     np.linalg.norm(AP - AP.T) / c, np.linalg.norm(PA - PA.T) / c]) / tol


def check_full_rank(A64, B64, X, rank, dtype):
    """The full-rank checks of one matrix; returns the worst fraction of (the
    backward limit, the forward bound)."""
    m, n = A64.shape
    k = min(m, n)
    tol = tol_of(k, dtype)
    assert rank == k, f"rank {rank} of a full-rank {m} x {n} matrix"
    Xref = np.linalg.lstsq(A64, B64, rcond=None)[0]
    fb = float(np.max(backward_errors(A64, X, B64)) / tol)
    ff = float(np.max(forward_fractions(A64, X, B64, Xref, tol)))
    assert fb <= 1, f"backward error is {fb:.2f} of its limit"
    assert ff <= 1, f"forward error is {ff:.2f} of Wedin's bound"
    return fb, ff


def check_deficient(A64, B64, X, rank, r, dtype):
    """The rank-deficient checks of one matrix; returns the fractions of (the
    null-space limit, the forward bound)."""
    m, n = A64.shape
    rcond = DEFICIENT_RCOND[dtype]
    U, sv, Vh = np.linalg.svd(A64)
    # the gap, from the reference alone: the cutoff is nowhere near a singular value
    assert sv[r - 1] / sv[0] >= 10 * rcond and sv[r] / sv[0] <= rcond / 10, (sv[r - 1] / sv[0], sv[r] / sv[0])
    assert rank == r, f"rank {rank} != {r}"
    X = np.asarray(X, dtype=np.float64)
    lim = mid_limits(n, dtype)
    V0 = Vh[r:].T
    fn = float(np.max(np.linalg.norm(V0.T @ X, axis=0) / np.linalg.norm(X, axis=0)) / lim[2])
    Xref = np.linalg.lstsq(A64, B64, rcond=rcond)[0]
    ff = float(np.max(forward_fractions(A64, X, B64, Xref, lim[1] + lim[2], kappa=sv[0] / sv[r - 1], sv=sv)))
    assert fn <= 1, f"null-space component is {fn:.2f} of its limit"
    assert ff <= 1, f"forward error is {ff:.2f} of Wedin's bound"
    return fn, ff


def check_pinv(A64, P, dtype):
    """Penrose conditions and the distance to float64 pinv, column by column
    under the forward bound of the identity's columns; returns the fractions."""
    m, n = A64.shape
    tol = tol_of(min(m, n), dtype)
    assert P.shape == (n, m)
    fp = float(np.max(penrose_fractions(A64, P, tol)))
    ff = float(np.max(forward_fractions(A64, P, np.eye(m), np.linalg.pinv(A64), tol)))
    assert fp <= 1, f"a Penrose condition is at {fp:.2f} of its limit"
    assert ff <= 1, f"distance to pinv is {ff:.2f} of Wedin's bound"
    return fp, ff
