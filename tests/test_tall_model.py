"""The numpy model of the batched tall SVD (tests/tall_model.py: blocked
Householder QR, jacobi_model.jacobi_svd on R, the reflectors back onto
[U_R; 0]) against numpy.linalg.svd of the float64 input, in float64 and
float32, at the shapes tests/test_gpu_svd_tall_batched.py runs on the GPU.

The limits are jacobi_model.LIMITS, unchanged (1e-13 / 2e-13 / 1e-12 in fp64,
2e-5 / 5e-5 / 5e-4 in fp32) and 1e-13 / 2e-5 relative on the graded golden
set: this test shows that the method alone -- this project's own Householder
front end, not LAPACK's -- stays inside them."""
import os

import numpy as np
import pytest

from jacobi_model import check_svd, rank_deficient
from tall_model import GPU_SHAPES, apply_q, row_block, tall_qr, tall_svd, uniform_batch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DT = {"f64": np.float64, "f32": np.float32}

SHAPES = GPU_SHAPES


def test_row_block_per_column_class():
    assert [row_block(n) for n in (1, 16, 17, 32, 33, 64)] == [256, 256, 256, 256, 128, 128]
    assert len(SHAPES) == len(set(SHAPES))
    for m, n in ((256, 1), (257, 1), (128, 64), (129, 64), (193, 64), (2 * 128 + 64 + 1, 64), (2 * 256 + 17 + 1, 17)):
        assert (m, n) in SHAPES


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("m,n", SHAPES, ids=[f"{m}x{n}" for m, n in SHAPES])
def test_model_against_numpy(m, n, sfx):
    dtype = DT[sfx]
    A64 = uniform_batch(m, n, 1)[0].astype(dtype).astype(np.float64)   # the rounded input is the matrix decomposed
    U, S, V, info = tall_svd(A64, dtype=dtype)
    assert U.dtype == dtype and S.dtype == dtype and V.dtype == dtype
    assert U.shape == (m, n) and info == 0
    e = check_svd(A64, U, S, V, dtype)
    print(f"{m}x{n} {sfx}: values {e[0]:.2e} reconstruction {e[1]:.2e} V {e[2]:.2e} U {e[3]:.2e}")


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_model_on_degenerate_inputs(sfx):
    dtype = DT[sfx]
    rng = np.random.default_rng(31)
    Z = np.zeros((200, 24))
    U, S, V, info = tall_svd(Z, dtype=dtype)
    assert info == 0 and np.all(S == 0) and np.all(U == 0)
    Id = np.zeros((200, 24))
    Id[:24] = np.eye(24)
    for A in (rank_deficient(rng, 200, 24), Id, rank_deficient(rng, 300, 24)):
        A64 = A.astype(dtype).astype(np.float64)
        U, S, V, info = tall_svd(A64, dtype=dtype)
        assert info == 0
        check_svd(A64, U, S, V, dtype)
    # a zero column: sigma = 0 and a zero column of U (the last one: S is descending)
    A = rng.uniform(0, 5, (300, 8))
    A[:, 3] = 0
    U, S, V, info = tall_svd(A, dtype=dtype)
    assert S[-1] == 0 and np.all(U[:, -1] == 0) and S[-2] > 0


def test_qr_factor_is_a_qr_factorisation():
    """R upper triangular, Q orthonormal, Q R = A, over three row blocks of 40."""
    A = np.random.default_rng(7).uniform(-1, 1, (100, 12))
    R, blocks = tall_qr(A, rb=40)
    assert [b[0] for b in blocks] == [0, 40, 80] and blocks[-1][1].shape == (20, 12)
    assert np.array_equal(R, np.triu(R))
    Q = apply_q(blocks, np.eye(12), 100)
    assert np.linalg.norm(Q.T @ Q - np.eye(12)) <= 1e-14
    assert np.linalg.norm(Q @ R - A) <= 1e-14 * np.linalg.norm(A)


@pytest.mark.parametrize("sfx,factor", [("f64", 1e150), ("f64", 1e-150), ("f32", 1e18), ("f32", 1e-18)])
def test_running_scale_covers_the_range(sfx, factor):
    """Squares of these entries overflow / underflow; a power of two scales S exactly."""
    dtype = DT[sfx]
    A = np.random.default_rng(71).uniform(1, 2, (300, 16)).astype(dtype)
    k = int(np.round(np.log2(factor)))
    S0 = tall_svd(A, dtype=dtype)[1]
    U, S, V, info = tall_svd(np.ldexp(A, k), dtype=dtype)
    assert info == 0 and np.array_equal(S, np.ldexp(S0, k))
    As = (A.astype(np.float64) * factor).astype(dtype)
    U, S, V, info = tall_svd(As, dtype=dtype)
    assert info == 0
    check_svd(As.astype(np.float64), U, S, V, dtype)


def test_scale_grows_with_a_later_block():
    """The largest entry arrives in the second block: R is rescaled, nothing is lost."""
    A = np.random.default_rng(9).uniform(0, 5, (300, 16))
    A[256:] *= 2.0 ** 200
    A[:, :4] *= 2.0 ** -100
    U, S, V, info = tall_svd(A)
    assert info == 0 and np.all(np.isfinite(S))
    check_svd(A, U, S, V, np.float64)


def test_non_finite_input_is_all_nan():
    A = np.ones((300, 8))
    A[250, 1] = np.inf
    U, S, V, info = tall_svd(A)
    assert info == 2
    assert np.all(np.isnan(U)) and np.all(np.isnan(S)) and np.all(np.isnan(V))


def test_model_against_the_graded_golden_set():
    g = np.load(os.path.join(GOLDEN, "batched_graded_tall.npz"))
    for sfx, lim in (("f64", 1e-13), ("f32", 2e-5)):
        A, ref = g[f"A_{sfx}"], g[f"S_{sfx}"]
        assert A.dtype == DT[sfx] and A.shape == (4, 300, 16) and ref.shape == (4, 16)
        worst = 0.0
        for i in range(A.shape[0]):
            S, info = tall_svd(A[i], dtype=DT[sfx])[1::2]
            assert info == 0
            worst = max(worst, float(np.max(np.abs(S.astype(np.float64) - ref[i]) / ref[i])))
        print(f"graded tall {sfx}: worst relative error {worst:.2e}")
        assert worst <= lim
