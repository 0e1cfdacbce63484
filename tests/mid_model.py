"""TEST INFRASTRUCTURE: the checks of the batched mid-size SVD
(brd_svd_mid_batched_*, 65 to 128 columns; DESIGN.md "Batched mid-size SVD").

The method is that of tests/jacobi_model.py, which stays the executable
specification.  What changes beyond 64 columns is the limits: a column takes
part in n - 1 rotations per sweep, each rotation adds O(eps), and the sweep
count barely grows, so the limits of jacobi_model.LIMITS are multiplied by
max(1, n / 64).
"""
from __future__ import annotations

import numpy as np

from jacobi_model import LIMITS

# relative error of every singular value of a graded matrix (the golden limit
# of tests/test_gpu_svd_batched.py), before the n / 64 scaling
GRADED_LIMIT = {np.float64: 1e-13, np.float32: 2e-5}


def mid_limits(n, dtype):
    """(values, reconstruction, orthogonality) limits at n columns."""
    f = max(1.0, n / 64.0)
    return tuple(f * x for x in LIMITS[dtype])


def graded_limit(n, dtype):
    return GRADED_LIMIT[dtype] * max(1.0, n / 64.0)


def rank_deficient_mid(rng, m=128, n=100):
    """A duplicated column, a zero column and a combination of two others."""
    A = rng.uniform(0, 5, (m, n))
    A[:, 70] = A[:, 2]
    A[:, 91] = 0.0
    A[:, 66] = 0.5 * A[:, 4] - 2.0 * A[:, 85]
    return A


def check_svd_mid(A64, U, S, V, dtype):
    """The four measures of jacobi_model.check_svd against numpy's float64 SVD
    of A64, under the limits scaled by max(1, n / 64); returns them."""
    m, n = A64.shape
    lim_s, lim_r, lim_o = mid_limits(n, dtype)
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
