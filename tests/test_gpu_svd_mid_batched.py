"""Batched SVD of mid-size matrices on the GPU (brd_svd_mid_batched_*,
svdsolver_amd.svd_mid_batched): 65 to 128 columns, n <= m <= 128, one-sided
Jacobi, one launch, one workgroup per matrix.

Reference: numpy.linalg.svd in float64 on the CPU, of the input rounded to the
dtype under test.  Limits: tests/mid_model.py, jacobi_model.LIMITS times
n / 64; at 128 columns (fp64 / fp32)
    max|S - S_ref|                <= 2e-13 / 4e-5 * sigma_1
    |U S V^T - A|_F               <= 4e-13 / 1e-4 * |A|_F
    |V^T V - I|_F, |U^T U - I|_F  <= 2e-12 / 1e-3
tests/test_mid_model.py shows that the numpy model of the method stays at or
below 0.26 of them.  Everything runs in this one process.
"""
import ctypes
import os

import numpy as np
import pytest

import svdsolver_amd as S
from mid_model import check_svd_mid, graded_limit

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
SHAPES = [(65, 65), (66, 65), (72, 72), (97, 96), (100, 72), (128, 65), (128, 96), (128, 127), (128, 128),
          (65, 128), (96, 100)]   # the last two are wide: decomposed as their transposes


def _run(A, fn=None, **kw):
    """svd_mid_batched (or fn) on a numpy batch; numpy results."""
    import torch
    out = (fn or S.svd_mid_batched)(torch.from_numpy(np.ascontiguousarray(A)).cuda(), **kw)
    if isinstance(out, tuple):
        return tuple(o.cpu().numpy() for o in out)
    return out.cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check_batch(A, U, Sv, Vh, dtype):
    """Every matrix against its own reference; a wide one as its transpose."""
    worst = np.zeros(4)
    for i in range(A.shape[0]):
        A64 = A[i].astype(np.float64)
        if A64.shape[0] >= A64.shape[1]:
            e = check_svd_mid(A64, U[i], Sv[i], Vh[i].T, dtype)
        else:
            e = check_svd_mid(A64.T, Vh[i].T, Sv[i], U[i], dtype)
        worst = np.maximum(worst, e)
    return worst


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("m,n", SHAPES, ids=[f"{m}x{n}" for m, n in SHAPES])
def test_shapes_against_numpy(m, n, sfx):
    dtype = DT[sfx]
    k = min(m, n)
    A = np.random.default_rng(1000 * m + n).uniform(0, 5, (3, m, n)).astype(dtype)
    U, Sv, Vh, info = _run(A, check=False)
    assert U.shape == (3, m, k) and Sv.shape == (3, k) and Vh.shape == (3, k, n)
    assert U.dtype == dtype and Sv.dtype == dtype and Vh.dtype == dtype
    assert np.array_equal(info, np.zeros(3, np.int32))
    w = _check_batch(A, U, Sv, Vh, dtype)
    print(f"{m}x{n} {sfx}: values {w[0]:.2e} reconstruction {w[1]:.2e} V {w[2]:.2e} U {w[3]:.2e}")
    # values only: the same rotations of G, so bitwise the values of the vectors call
    Sv2, info2 = _run(A, fn=S.svdvals_mid_batched, check=False)
    assert np.array_equal(info2, np.zeros(3, np.int32))
    assert _same_bits(Sv2, Sv), "values-only call differs from the vectors call"


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("m,n", [(128, 64), (64, 64), (17, 16)])
def test_small_matrices_forward_to_svd_batched_bitwise(m, n, sfx):
    A = np.random.default_rng(1000 * m + n).uniform(0, 5, (3, m, n)).astype(DT[sfx])
    mid = _run(A, check=False)
    small = _run(A, fn=S.svd_batched, check=False)
    for a, b in zip(mid, small):
        assert _same_bits(a, b)
    assert _same_bits(_run(A, fn=S.svdvals_mid_batched), _run(A, fn=S.svdvals_batched))


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_mixed_batch_each_matrix_against_its_own_reference(sfx):
    """300 different 80 x 72 matrices (more workgroups than CUs): batch indexing."""
    dtype = DT[sfx]
    rng = np.random.default_rng(31)
    A = rng.uniform(0, 5, (300, 80, 72))
    A *= rng.uniform(0.1, 10.0, (300, 1, 1))
    A[0] = 0.0
    A[150] = _rank_deficient_80x72(rng)
    A[299] = 0.0
    A[299, :72, :] = np.eye(72)
    A = A.astype(dtype)
    U, Sv, Vh, info = _run(A, check=False)
    assert np.array_equal(info, np.zeros(300, np.int32))
    _check_batch(A, U, Sv, Vh, dtype)
    assert np.all(Sv[0] == 0) and np.all(U[0] == 0)
    assert np.allclose(Sv[299], 1.0, rtol=0, atol=1e-6)
    assert Sv[150][-1] <= 72 * np.finfo(dtype).eps * Sv[150][0]


def _rank_deficient_80x72(rng):
    """A duplicated column, a zero column and a combination of two others."""
    A = rng.uniform(0, 5, (80, 72))
    A[:, 67] = A[:, 2]
    A[:, 11] = 0.0
    A[:, 69] = 0.5 * A[:, 4] - 2.0 * A[:, 65]
    return A


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_layout_padding_untouched_and_input_unchanged(sfx):
    """The C ABI at 70 x 66 with lda = n + 3, ldu = n + 1, ldv = n + 2 and odd
    batch strides.  In fp64 the working copy of V lives in the caller's V
    block: this is the test that sees it write outside the n x n entries."""
    import torch
    dtype = DT[sfx]
    batch, m, n = 5, 70, 66
    lda, ldu, ldv = n + 3, n + 1, n + 2
    sa, su, sv = m * lda + 7, m * ldu + 5, n * ldv + 3
    sent = -777.0
    rng = np.random.default_rng(41)
    dense = rng.uniform(0, 5, (batch, m, n)).astype(dtype)
    Abuf = np.full(batch * sa, sent, dtype=dtype)
    for i in range(batch):
        for r in range(m):
            o = i * sa + r * lda
            Abuf[o:o + n] = dense[i, r]
    dA = torch.from_numpy(Abuf).cuda()
    dS = torch.full((batch * n + 4,), sent, dtype=dA.dtype, device="cuda")
    dU = torch.full((batch * su,), sent, dtype=dA.dtype, device="cuda")
    dV = torch.full((batch * sv,), sent, dtype=dA.dtype, device="cuda")
    dI = torch.full((batch + 2,), -9, dtype=torch.int32, device="cuda")
    S.lib.brd_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    fn = getattr(S.lib, f"brd_svd_mid_batched_{sfx}")
    rc = fn(dA.data_ptr(), batch, m, n, lda, sa, dS.data_ptr(), dU.data_ptr(), ldu, su, dV.data_ptr(), ldv, sv,
            dI.data_ptr(), 0)
    assert rc == 0, S.lib.brd_last_error()
    assert np.array_equal(dA.cpu().numpy().view(np.uint8), Abuf.view(np.uint8)), "A was written"
    hS, hU, hV, hI = dS.cpu().numpy(), dU.cpu().numpy(), dV.cpu().numpy(), dI.cpu().numpy()
    assert np.array_equal(hI, np.array([0] * batch + [-9, -9], np.int32))
    assert np.all(hS[batch * n:] == sent)
    umask = np.zeros(batch * su, dtype=bool)
    vmask = np.zeros(batch * sv, dtype=bool)
    U = np.empty((batch, m, n), dtype)
    V = np.empty((batch, n, n), dtype)
    for i in range(batch):
        for r in range(m):
            o = i * su + r * ldu
            U[i, r] = hU[o:o + n]
            umask[o:o + n] = True
        for r in range(n):
            o = i * sv + r * ldv
            V[i, r] = hV[o:o + n]
            vmask[o:o + n] = True
    assert np.all(hU[~umask] == sent) and np.all(hV[~vmask] == sent), "padding was written"
    for i in range(batch):
        check_svd_mid(dense[i].astype(np.float64), U[i], hS[i * n:(i + 1) * n], V[i], dtype)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("m,n", [(128, 128), (97, 96)])
def test_two_runs_are_bit_identical(m, n, sfx):
    import torch
    A = np.random.default_rng(51).uniform(0, 5, (3, m, n)).astype(DT[sfx])
    dA = torch.from_numpy(A).cuda()
    U1, S1, Vh1 = S.svd_mid_batched(dA)
    U2, S2, Vh2 = S.svd_mid_batched(dA)
    for a, b in ((U1, U2), (S1, S2), (Vh1, Vh2)):
        assert _same_bits(a.cpu().numpy(), b.cpu().numpy()), "two identical calls differ"
    U3, S3, Vh3, info = S.svd_mid_batched(dA, check=False, sync=False)
    torch.cuda.synchronize()
    assert torch.equal(U3, U1) and torch.equal(S3, S1) and torch.equal(Vh3, Vh1)
    assert int(info.abs().sum()) == 0
    # a single matrix: shaped like torch.linalg.svd(A, full_matrices=False)
    u, s, vh = S.svd_mid_batched(dA[1])
    assert u.shape == (m, n) and s.shape == (n,) and vh.shape == (n, n)
    assert torch.equal(s, S1[1]) and torch.equal(u, U1[1]) and torch.equal(vh, Vh1[1])


@pytest.mark.parametrize("sfx,k", [("f64", 500), ("f64", -500), ("f32", 60), ("f32", -60)])
def test_power_of_two_scaling_is_exact(sfx, k):
    """Squares of these entries overflow / underflow; the kernel scales by a
    power of two first, so S scales exactly and U and V do not change."""
    dtype = DT[sfx]
    A = np.random.default_rng(71).uniform(1, 2, (2, 100, 80)).astype(dtype)
    U0, S0, Vh0 = _run(A)
    As = np.ldexp(A, k)
    assert As.dtype == dtype and np.all(np.isfinite(As)) and np.all(As != 0)
    U, Sv, Vh, info = _run(As, check=False)
    assert np.array_equal(info, np.zeros(2, np.int32))
    assert np.array_equal(Sv, np.ldexp(S0, k)), "a power of two does not scale S exactly"
    assert _same_bits(U, U0) and _same_bits(Vh, Vh0)
    _check_batch(As, U, Sv, Vh, dtype)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_non_finite_matrices_are_flagged_and_isolated(sfx):
    dtype = DT[sfx]
    A = np.random.default_rng(81).uniform(0, 5, (4, 128, 128)).astype(dtype)
    clean = _run(A, check=False)
    assert clean[3].tolist() == [0, 0, 0, 0]
    B = A.copy()
    B[1, 77, 101] = np.nan
    B[3, 127, 0] = np.inf
    U, Sv, Vh, info = _run(B, check=False)
    assert info.tolist() == [0, 2, 0, 2]
    for i in (1, 3):
        assert np.all(np.isnan(U[i])) and np.all(np.isnan(Sv[i])) and np.all(np.isnan(Vh[i]))
    for i in (0, 2):
        assert _same_bits(U[i], clean[0][i]) and _same_bits(Sv[i], clean[1][i]) and _same_bits(Vh[i], clean[2][i])
    # check=True leaves the NaNs in place and does not raise for info 2
    S2 = _run(B, compute_uv=False)
    assert np.all(np.isnan(S2[[1, 3]])) and _same_bits(S2[[0, 2]], clean[1][[0, 2]])


def test_graded_matrices_relative_accuracy(golden_dir):
    """A = B D with cond(B) = 20 and D over 2^-40 (fp64) / 2^-20 (fp32): every
    singular value to relative accuracy, limit 1e-13 n/64 / 2e-5 n/64 (the
    model: at most 2.3e-14 / 8.0e-6).  LAPACK in float64 loses the small ones
    of the fp64 128 x 128 matrix."""
    g = np.load(os.path.join(golden_dir, "batched_graded_mid.npz"))
    for sfx, dtype in DT.items():
        for i in range(3):
            A, ref = g[f"A_{sfx}_{i}"], g[f"S_{sfx}_{i}"]
            assert A.dtype == dtype
            n = A.shape[1]
            U, Sv, Vh, info = _run(A[None], check=False)
            assert info.tolist() == [0]
            rel = np.max(np.abs(Sv[0].astype(np.float64) - ref) / ref)
            print(f"graded {sfx} {A.shape[0]}x{n}: worst relative error {rel:.2e} (limit {graded_limit(n, dtype):.1e})")
            assert rel <= graded_limit(n, dtype)
            assert _same_bits(_run(A[None], compute_uv=False), Sv)
    A, ref = g["A_f64_0"], g["S_f64_0"]
    lapack = np.max(np.abs(np.linalg.svd(A, compute_uv=False) - ref) / ref)
    print(f"LAPACK float64 on the fp64 128x128 matrix: worst relative error {lapack:.2e}")
    assert lapack > graded_limit(128, np.float64)


def test_profile_kind_and_size_limits():
    import torch
    S.profile_enable(True)
    S.profile_reset()
    S.svd_mid_batched(torch.rand((4, 100, 96), dtype=torch.float64, device="cuda"))
    q = S.profile_query("svd_mid_batched")
    assert q["launches"] == 1 and q["ms"] > 0
    assert q["bytes"] == 4 * (9600 + 96 + 9600 + 96 * 96) * 8 + 4 * 4
    assert S.profile_query("svd_batched")["launches"] == 0
    # values only, fp32, and a forwarded call: one entry each
    S.profile_reset()
    S.svdvals_mid_batched(torch.rand((3, 70, 66), dtype=torch.float32, device="cuda"))
    S.svd_mid_batched(torch.rand((4, 8, 8), dtype=torch.float64, device="cuda"))
    q = S.profile_query("svd_mid_batched")
    S.profile_enable(False)
    assert q["launches"] == 2
    assert q["bytes"] == 3 * (70 * 66 + 66) * 4 + 3 * 4 + 4 * (64 + 8 + 64 + 64) * 8 + 4 * 4
    with pytest.raises(S.BrdError) as ei:
        S.svd_mid_batched(torch.zeros((2, 129, 8), device="cuda"))
    assert ei.value.code == -5
    assert "128 x 128" in str(ei.value)
