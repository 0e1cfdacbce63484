"""TEST INFRASTRUCTURE: numpy model of the one-sided Jacobi (Hestenes) SVD
that brd_svd_batched.hip implements on the GPU (DESIGN.md "Batched small
SVD").

Not the product path -- it is the executable specification of the method: the
same round-robin pair schedule, rotation threshold and formulas, sweep cap,
descending rank sort with ties broken by column index, and zero-column rule.
It works in any numpy float dtype (np.longdouble included: the golden values
of tests/golden/batched_graded.npz come from it), and it is itself checked
against numpy.linalg.svd (tests/test_jacobi_model.py), which shows that the
method alone stays inside the limits the GPU tests use.

Only the order of the floating-point sums differs from the kernel (numpy's
pairwise sum against the kernel's strided loop and shuffle tree).
"""
from __future__ import annotations

import numpy as np

MAX_SWEEPS = 30   # xGESVJ's cap


def step_pairs(n: int, k: int):
    """Pairs (p < q) of step k (0 .. np-2) of the round-robin tournament on
    np = n rounded up to even players.  Player np-1 meets k; (k + j) meets
    (k - j) mod (np - 1).  For odd n the dummy is player np-1 and its pair is
    dropped."""
    npl = (n + 1) & ~1
    P, Q = [], []
    if n % 2 == 0:
        P.append(k)
        Q.append(npl - 1)
    for j in range(1, npl // 2):
        a = (k + j) % (npl - 1)
        b = (k - j) % (npl - 1)
        P.append(min(a, b))
        Q.append(max(a, b))
    return np.array(P, dtype=np.intp), np.array(Q, dtype=np.intp)


def jacobi_svd(A, dtype=None, scale: bool = True):
    """One-sided Jacobi SVD of the m x n matrix A (m >= n) in ``dtype``.

    Returns (U, S, V, info, sweeps): A = U diag(S) V^T, S descending, U m x n,
    V n x n; info 0 (converged), 1 (sweep cap; the current iterate) or 2
    (non-finite input; everything NaN).  ``scale``: the power-of-two scaling
    of the kernel (the largest |a_ij| into [1/2, 1))."""
    dt = np.dtype(dtype if dtype is not None else np.asarray(A).dtype)
    G = np.array(A, dtype=dt, copy=True)
    m, n = G.shape
    assert m >= n >= 1
    if not np.all(np.isfinite(G)):
        nan = np.full((), np.nan, dtype=dt)
        return (np.full((m, n), nan), np.full(n, nan), np.full((n, n), nan), 2, 0)
    eps = np.finfo(dt).eps
    ex = 0
    mx = np.max(np.abs(G))
    if scale and mx > 0:
        ex = int(np.frexp(mx)[1])
        G = np.ldexp(G, -ex).astype(dt)
    V = np.eye(n, dtype=dt)
    tol = np.sqrt(dt.type(m)) * eps
    npl = (n + 1) & ~1
    one, two = dt.type(1), dt.type(2)
    info, sweeps = 1, 0
    for _ in range(MAX_SWEEPS):
        sweeps += 1
        rotated = False
        for k in range(npl - 1):
            P, Q = step_pairs(n, k)
            if P.size == 0:
                continue
            x, y = G[:, P], G[:, Q]
            al = np.sum(x * x, axis=0)
            be = np.sum(y * y, axis=0)
            ga = np.sum(x * y, axis=0)
            rot = np.abs(ga) > tol * np.sqrt(al) * np.sqrt(be)
            if not np.any(rot):
                continue
            rotated = True
            P, Q, x, y = P[rot], Q[rot], x[:, rot], y[:, rot]
            al, be, ga = al[rot], be[rot], ga[rot]
            with np.errstate(over="ignore"):
                zeta = (be - al) / (two * ga)
                t = np.copysign(one, zeta) / (np.abs(zeta) + np.sqrt(one + zeta * zeta))
            c = one / np.sqrt(one + t * t)
            s = c * t
            G[:, P] = c * x - s * y
            G[:, Q] = s * x + c * y
            vx, vy = V[:, P], V[:, Q]
            V[:, P] = c * vx - s * vy
            V[:, Q] = s * vx + c * vy
        if not rotated:
            info = 0
            break
    sig = np.sqrt(np.sum(G * G, axis=0))
    # descending, ties by column index: rank_j = #{i: s_i > s_j or (s_i == s_j and i < j)}
    order = np.lexsort((np.arange(n), -sig))
    sig, G, V = sig[order], G[:, order], V[:, order]
    U = np.zeros((m, n), dtype=dt)
    nz = sig > 0
    U[:, nz] = G[:, nz] / sig[nz]
    S = np.ldexp(sig, ex).astype(dt)
    return U, S, V, info, sweeps


# ---------------------------------------------------------------------------
# the checks shared by the model tests and the GPU tests
# ---------------------------------------------------------------------------
# fp64 / fp32: max|S - S_ref| / s_1, |U S V^T - A|_F / |A|_F, |V^T V - I|_F (and U)
LIMITS = {np.float64: (1e-13, 2e-13, 1e-12), np.float32: (2e-5, 5e-5, 5e-4)}


def rank_deficient(rng, m=40, n=24):
    """A duplicated column, a zero column and a combination of two others."""
    A = rng.uniform(0, 5, (m, n))
    A[:, 7] = A[:, 2]
    A[:, 11] = 0.0
    A[:, 19] = 0.5 * A[:, 4] - 2.0 * A[:, 15]
    return A


def check_svd(A64, U, S, V, dtype):
    """The four measures against numpy's float64 SVD of A64; returns them."""
    lim_s, lim_r, lim_o = LIMITS[dtype]
    m, n = A64.shape
    U, S, V = (np.asarray(x, dtype=np.float64) for x in (U, S, V))
    ref = np.linalg.svd(A64, compute_uv=False)
    s1 = ref[0]
    assert np.all(np.diff(S) <= 0), "descending order"
    e_s = np.max(np.abs(S - ref)) / s1 if s1 > 0 else np.max(np.abs(S))
    na = np.linalg.norm(A64)
    e_r = np.linalg.norm((U * S) @ V.T - A64) / na if na > 0 else np.linalg.norm((U * S) @ V.T)
    e_v = np.linalg.norm(V.T @ V - np.eye(n))
    keep = S > n * np.finfo(dtype).eps * s1
    Uk = U[:, keep]
    e_u = np.linalg.norm(Uk.T @ Uk - np.eye(Uk.shape[1]))
    assert e_s <= lim_s, f"values {e_s:.2e}"
    assert e_r <= lim_r, f"reconstruction {e_r:.2e}"
    assert e_v <= lim_o, f"V orthogonality {e_v:.2e}"
    assert e_u <= lim_o, f"U orthogonality {e_u:.2e}"
    return e_s, e_r, e_v, e_u
