"""The numpy model of the batched least squares (tests/ls_model.py: the SVD of
the route the library takes, then the solve kernel's three phases with its
cutoff rule, all in working precision) against numpy.linalg.lstsq / pinv in
float64 on the input rounded to the dtype, at the shapes
tests/test_gpu_lstsq_batched.py runs on the GPU.

This shows, without a GPU, that the method alone stays inside every limit of
ls_model at every one of those shapes.  Worst fractions of a limit seen (first
matrix of every batch; fp64 / fp32):
    full rank    backward 0.0002 / 0.0003    forward 0.0001 / below 0.0001
    transposed   backward 0.0003 / 0.0006    forward 0.0001 / 0.0002
    deficient    null space 0.0021 / 0.0019  forward 0.0001 / 0.0001
    pinv         Penrose 0.0003 / 0.0006     distance to pinv 0.0002 / 0.0002
The limits are the SVD factors' own (1e-13 to 1e-12 in fp64, 1e-5 to 1e-3 in
fp32, about 10^3 eps), so a solve that is backward stable to a few eps sits at
a thousandth of them.
"""
import numpy as np
import pytest

import ls_model as M

SFX = ["f64", "f32"]


def _ids(shapes):
    return ["x".join(str(v) for v in s) for s in shapes]


def _rounded(dtype, *arrays):
    return tuple(a.astype(dtype).astype(np.float64) for a in arrays)


def test_shape_grid_is_the_one_the_gpu_test_needs():
    shapes = {(m, n) for m, n, _ in M.LS_SHAPES}
    assert shapes == {(5, 3), (64, 64), (128, 64), (300, 33), (128, 96), (128, 128), (129, 65), (300, 72), (257, 128)}
    for mn in shapes:   # nrhs = 1 and one other value
        ks = sorted(k for m, n, k in M.LS_SHAPES if (m, n) == mn)
        assert len(ks) == 2 and ks[0] == 1 and ks[1] in (2, 16, 17, 33)
    for k in (1, 2, 16, 17, 33):   # at one n <= 64 and one n > 64
        assert any(n <= 64 for _, n, kk in M.LS_SHAPES if kk == k)
        assert any(n > 64 for _, n, kk in M.LS_SHAPES if kk == k)
    assert {(m, n) for m, n, _ in M.WIDE_SHAPES} == {(72, 400), (3, 5)}
    assert M.PINV_SHAPES == [(128, 128), (300, 72), (72, 400)]
    assert M.DEFICIENT == [(300, 72, 40), (200, 100, 60), (40, 16, 9)]


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("m,n,nrhs", M.LS_SHAPES + M.WIDE_SHAPES, ids=_ids(M.LS_SHAPES + M.WIDE_SHAPES))
def test_model_full_rank(m, n, nrhs, sfx):
    dtype = M.DT[sfx]
    A, B = M.uniform_system(m, n, nrhs, 1)
    A64, B64 = _rounded(dtype, A[0], B[0])
    X, rank, S = M.model_lstsq(A64, B64, None, dtype)
    assert X.dtype == dtype and X.shape == (n, nrhs) and S.shape == (min(m, n),)
    fb, ff = M.check_full_rank(A64, B64, X, rank, dtype)
    print(f"{m}x{n} nrhs {nrhs} {sfx}: backward {fb:.4f} forward {ff:.4f} of the limit")


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("m,n,r", M.DEFICIENT, ids=_ids(M.DEFICIENT))
def test_model_rank_deficient(m, n, r, sfx):
    dtype = M.DT[sfx]
    A, B = M.deficient_system(m, n, r, 1)
    A64, B64 = _rounded(dtype, A[0], B[0])
    X, rank, _ = M.model_lstsq(A64, B64, M.DEFICIENT_RCOND[dtype], dtype)
    fn, ff = M.check_deficient(A64, B64, X, rank, r, dtype)
    print(f"{m}x{n} rank {r} {sfx}: null space {fn:.4f} forward {ff:.4f} of the limit")


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("m,n", M.PINV_SHAPES, ids=_ids(M.PINV_SHAPES))
def test_model_pinv(m, n, sfx):
    dtype = M.DT[sfx]
    (A64,) = _rounded(dtype, M.uniform_system(m, n, 1, 1)[0][0])
    P, rank, _ = M.model_lstsq(A64, None, None, dtype)
    assert rank == min(m, n)
    fp, ff = M.check_pinv(A64, P, dtype)
    print(f"pinv {m}x{n} {sfx}: Penrose {fp:.4f} distance {ff:.4f} of the limit")


@pytest.mark.parametrize("sfx", SFX)
def test_model_rcond_rules(sfx):
    dtype = M.DT[sfx]
    A, B = M.uniform_system(40, 16, 2, 1)
    A64, B64 = _rounded(dtype, A[0], B[0])
    assert M.model_lstsq(A64, B64, 0.0, dtype)[1] == 16          # every non-zero value is kept
    for rc in (1.0, 2.0):                                          # sigma_j > rcond sigma_1 never holds
        X, rank, _ = M.model_lstsq(A64, B64, rc, dtype)
        assert rank == 0 and np.all(X == 0)
    X, rank, S = M.model_lstsq(np.zeros((40, 16)), B64, None, dtype)
    assert rank == 0 and np.all(X == 0) and np.all(S == 0)
    A64[:, 5] = 0                                                 # one exact zero value: rcond = 0 drops only it
    assert M.model_lstsq(A64, B64, 0.0, dtype)[1] == 15
    A64[3, 3] = np.nan
    X, rank, _ = M.model_lstsq(A64, B64, None, dtype)
    assert rank == -1 and np.all(np.isnan(X)) and X.shape == (16, 2)
