"""The numpy model of the batched tall mid-size SVD (tests/tall_mid_model.py:
tall_model.tall_qr at 128 rows per block, jacobi_model.jacobi_svd on R, the
reflectors back onto [U_R; 0]) against numpy.linalg.svd of the float64 input,
in float64 and float32, at the shapes tests/test_gpu_gesvd_batched.py runs on
the GPU.

The limits are mid_model.check_svd_mid's (jacobi_model.LIMITS x n / 64) and
mid_model.graded_limit on the graded golden set: this test shows that the
method alone stays inside them.  Worst measures seen, as fractions of their
limits: fp64 0.17 (values, 257 x 128), fp32 0.26 (V orthogonality, 255 x 127);
on the graded golden set 0.11 (fp64) and 0.24 (fp32)."""
import os

import numpy as np
import pytest

from mid_model import check_svd_mid, graded_limit, mid_limits, rank_deficient_mid
from tall_mid_model import GPU_SHAPES, RB, tall_mid_svd, uniform_batch
from tall_model import apply_q, tall_qr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DT = {"f64": np.float64, "f32": np.float32}


def test_shapes_cover_the_block_boundaries():
    assert RB == 128 and len(GPU_SHAPES) == len(set(GPU_SHAPES))
    assert all(m > 128 and m >= n and 65 <= n <= 128 for m, n in GPU_SHAPES)
    for m, n in ((129, 65), (129, 128), (RB + 128, 128), (RB + 128 + 1, 128), (2 * RB + 65 + 1, 65), (1000, 72),
                 (2049, 128)):
        assert (m, n) in GPU_SHAPES


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("m,n", GPU_SHAPES, ids=[f"{m}x{n}" for m, n in GPU_SHAPES])
def test_model_against_numpy(m, n, sfx):
    dtype = DT[sfx]
    A64 = uniform_batch(m, n, 1)[0].astype(dtype).astype(np.float64)   # the rounded input is the matrix decomposed
    U, S, V, info = tall_mid_svd(A64, dtype=dtype)
    assert U.dtype == dtype and S.dtype == dtype and V.dtype == dtype
    assert U.shape == (m, n) and info == 0
    e = check_svd_mid(A64, U, S, V, dtype)
    lim = mid_limits(n, dtype)
    frac = (e[0] / lim[0], e[1] / lim[1], e[2] / lim[2], e[3] / lim[2])
    print(f"{m}x{n} {sfx}: values {e[0]:.2e} reconstruction {e[1]:.2e} V {e[2]:.2e} U {e[3]:.2e}; "
          f"worst fraction of a limit {max(frac):.2f}")


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_model_on_degenerate_inputs(sfx):
    dtype = DT[sfx]
    rng = np.random.default_rng(31)
    Z = np.zeros((300, 100))
    U, S, V, info = tall_mid_svd(Z, dtype=dtype)
    assert info == 0 and np.all(S == 0) and np.all(U == 0)
    Id = np.zeros((300, 100))
    Id[:100] = np.eye(100)
    A = rank_deficient_mid(rng, 300, 100)
    for X in (A, Id):
        X64 = X.astype(dtype).astype(np.float64)
        U, S, V, info = tall_mid_svd(X64, dtype=dtype)
        assert info == 0
        check_svd_mid(X64, U, S, V, dtype)
    # the zero column of the rank-deficient matrix: sigma = 0 and a zero column of U
    U, S, V, info = tall_mid_svd(A, dtype=dtype)
    assert S[-1] == 0 and np.all(U[:, -1] == 0)


def test_qr_factor_is_a_qr_factorisation_at_this_block_height():
    A = np.random.default_rng(7).uniform(-1, 1, (300, 72))
    R, blocks = tall_qr(A, rb=RB)
    assert [b[0] for b in blocks] == [0, 128, 256] and blocks[-1][1].shape == (44, 72)
    assert np.array_equal(R, np.triu(R))
    Q = apply_q(blocks, np.eye(72), 300)
    assert np.linalg.norm(Q.T @ Q - np.eye(72)) <= 1e-13
    assert np.linalg.norm(Q @ R - A) <= 1e-14 * np.linalg.norm(A)


@pytest.mark.parametrize("row", [5, 200])   # the first row block and a later one
def test_non_finite_input_gives_nan_r_and_info_2(row):
    A = np.random.default_rng(3).uniform(0, 5, (300, 72))
    A[row, 9] = np.nan
    R, _ = tall_qr(A, rb=RB)
    assert np.all(np.isnan(R))
    U, S, V, info = tall_mid_svd(A)
    assert info == 2
    assert np.all(np.isnan(U)) and np.all(np.isnan(S)) and np.all(np.isnan(V))


def test_model_against_the_graded_golden_set():
    g = np.load(os.path.join(GOLDEN, "batched_graded_tall_mid.npz"))
    shapes = [(300, 72), (300, 72), (257, 128)]
    for sfx in ("f64", "f32"):
        worst = 0.0
        for i, (m, n) in enumerate(shapes):
            A, ref = g[f"A_{sfx}_{i}"], g[f"S_{sfx}_{i}"]
            assert A.dtype == DT[sfx] and A.shape == (m, n) and ref.shape == (n,) and ref.dtype == np.float64
            S, info = tall_mid_svd(A, dtype=DT[sfx])[1::2]
            assert info == 0
            rel = float(np.max(np.abs(S.astype(np.float64) - ref) / ref))
            assert rel <= graded_limit(n, DT[sfx])
            worst = max(worst, rel / graded_limit(n, DT[sfx]))
        print(f"graded tall mid {sfx}: worst relative error is {worst:.2f} of its limit")


def test_golden_file_is_no_larger_than_the_largest_fixture_before_it():
    mine = os.path.join(GOLDEN, "batched_graded_tall_mid.npz")
    others = [os.path.join(d, f) for d, _, fs in os.walk(GOLDEN) for f in fs]
    assert os.path.getsize(mine) <= max(os.path.getsize(p) for p in others if p != mine)
    assert os.path.getsize(mine) <= 1 << 20
