"""The numpy model of the batched one-sided Jacobi SVD (tests/jacobi_model.py)
against numpy.linalg.svd of the float64 input, in float64 and float32.

The limits are the ones tests/test_gpu_svd_batched.py applies to the kernel;
this test shows that the method alone stays inside them (a model of this kind
measured 3.9e-15 / 2.2e-6 on the values, 8.4e-15 / 5.6e-6 on the
reconstruction and 8.7e-14 / 7.0e-5 on the orthogonality at 128 x 64 and
64 x 64, in at most 11 sweeps: the limits allow 10-25x over that)."""
import numpy as np
import pytest

from jacobi_model import check_svd, jacobi_svd, rank_deficient, step_pairs


def model_inputs():
    rng = np.random.default_rng(2024)
    cases = [(f"uniform{m}x{n}", rng.uniform(0, 5, (m, n)))
             for m, n in ((1, 1), (5, 3), (17, 16), (33, 32), (64, 64), (100, 37), (128, 64))]
    cases.append(("rankdef40x24", rank_deficient(rng)))
    cases.append(("zeros8x8", np.zeros((8, 8))))
    cases.append(("identity16", np.eye(16)))
    return cases


CASES = model_inputs()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,A", CASES, ids=[c[0] for c in CASES])
def test_model_against_numpy(name, A, dtype):
    A64 = A.astype(dtype).astype(np.float64)   # the rounded input is the matrix decomposed
    U, S, V, info, sweeps = jacobi_svd(A64, dtype=dtype)
    assert U.dtype == dtype and S.dtype == dtype and V.dtype == dtype
    assert info == 0, f"sweep cap reached ({sweeps} sweeps)"
    check_svd(A64, U, S, V, dtype)


def test_zero_column_gives_zero_sigma_and_zero_u():
    U, S, V, info, _ = jacobi_svd(np.zeros((8, 8)))
    assert info == 0 and np.all(S == 0) and np.all(U == 0)
    assert np.array_equal(V, np.eye(8))


def test_non_finite_input_is_all_nan():
    A = np.ones((5, 3))
    A[2, 1] = np.nan
    U, S, V, info, sweeps = jacobi_svd(A)
    assert info == 2 and sweeps == 0
    assert np.all(np.isnan(U)) and np.all(np.isnan(S)) and np.all(np.isnan(V))


@pytest.mark.parametrize("n", [1, 2, 3, 7, 16, 37, 64])
def test_schedule_meets_every_pair_once(n):
    seen = set()
    for k in range(((n + 1) & ~1) - 1):
        P, Q = step_pairs(n, k)
        cols = np.concatenate([P, Q])
        assert len(set(cols.tolist())) == cols.size, "pairs of a step are disjoint"
        assert np.all(P < Q) and (cols.size == 0 or cols.max() < n)
        seen |= set(zip(P.tolist(), Q.tolist()))
    assert len(seen) == n * (n - 1) // 2


def test_longdouble_model_runs():
    A = np.random.default_rng(5).uniform(0, 5, (12, 7))
    U, S, V, info, _ = jacobi_svd(A, dtype=np.longdouble)
    assert S.dtype == np.longdouble and info == 0
    assert np.max(np.abs(S.astype(np.float64) - np.linalg.svd(A, compute_uv=False))) <= 1e-14 * float(S[0])
