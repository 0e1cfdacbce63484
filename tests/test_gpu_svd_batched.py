"""Batched SVD of small matrices on the GPU (brd_svd_batched_*,
svdsolver_amd.svd_batched): one-sided Jacobi, one launch for the whole batch.

Reference: numpy.linalg.svd in float64 on the CPU, of the input rounded to the
dtype under test.  Limits (fp64 / fp32), those of tests/test_jacobi_model.py,
where the numpy model of the method is shown to stay 10-25x inside them:
    max|S - S_ref|                <= 1e-13 / 2e-5 * sigma_1
    |U S V^T - A|_F               <= 2e-13 / 5e-5 * |A|_F
    |V^T V - I|_F, |U^T U - I|_F  <= 1e-12 / 5e-4   (U: columns with
                                                     sigma_j > n eps sigma_1)
"""
import ctypes
import os

import numpy as np
import pytest

import svdsolver_amd as S
from jacobi_model import check_svd, rank_deficient

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
SHAPES = [(1, 1), (2, 2), (3, 3), (5, 3), (16, 16), (17, 16), (17, 17), (33, 32), (33, 33), (64, 64), (100, 37),
          (128, 64)]


def _run(A, **kw):
    """svd_batched on a numpy batch; numpy results (Vh turned back into V)."""
    import torch
    out = S.svd_batched(torch.from_numpy(np.ascontiguousarray(A)).cuda(), **kw)
    if isinstance(out, tuple):
        out = tuple(o.cpu().numpy() for o in out)
    else:
        out = out.cpu().numpy()
    return out


def _check_batch(A, U, Sv, Vh, dtype):
    for i in range(A.shape[0]):
        check_svd(A[i].astype(np.float64), U[i], Sv[i], Vh[i].T, dtype)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("m,n", SHAPES, ids=[f"{m}x{n}" for m, n in SHAPES])
def test_shapes_against_numpy(m, n, sfx):
    dtype = DT[sfx]
    A = np.random.default_rng(1000 * m + n).uniform(0, 5, (3, m, n)).astype(dtype)
    U, Sv, Vh, info = _run(A, check=False)
    assert U.shape == (3, m, n) and Sv.shape == (3, n) and Vh.shape == (3, n, n)
    assert U.dtype == dtype and Sv.dtype == dtype and Vh.dtype == dtype
    assert np.array_equal(info, np.zeros(3, np.int32))
    _check_batch(A, U, Sv, Vh, dtype)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_mixed_batch_each_matrix_against_its_own_reference(sfx):
    """300 different 32 x 24 matrices (more workgroups than CUs): batch indexing."""
    dtype = DT[sfx]
    rng = np.random.default_rng(31)
    A = rng.uniform(0, 5, (300, 32, 24))
    A *= rng.uniform(0.1, 10.0, (300, 1, 1))
    A[0] = 0.0
    A[150] = rank_deficient(rng, 32, 24)
    A[299] = 0.0
    A[299, :24, :] = np.eye(24)
    A = A.astype(dtype)
    U, Sv, Vh, info = _run(A, check=False)
    assert np.array_equal(info, np.zeros(300, np.int32))
    _check_batch(A, U, Sv, Vh, dtype)
    assert np.all(Sv[0] == 0) and np.all(U[0] == 0)
    assert np.allclose(Sv[299], 1.0, rtol=0, atol=1e-6)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_layout_padding_untouched_and_input_unchanged(sfx):
    """The C ABI with lda = n + 3, batch stride m lda + 7, ldu = n + 1, ldv = n + 2."""
    import torch
    dtype = DT[sfx]
    batch, m, n = 5, 20, 12
    lda, ldu, ldv = n + 3, n + 1, n + 2
    sa, su, sv = m * lda + 7, m * ldu + 5, n * ldv + 3
    sent = -777.0
    rng = np.random.default_rng(41)
    dense = rng.uniform(0, 5, (batch, m, n)).astype(dtype)
    Abuf = np.full(batch * sa, sent, dtype=dtype)
    amask = np.zeros(batch * sa, dtype=bool)
    for i in range(batch):
        for r in range(m):
            o = i * sa + r * lda
            Abuf[o:o + n] = dense[i, r]
            amask[o:o + n] = True
    dA = torch.from_numpy(Abuf).cuda()
    dS = torch.full((batch * n + 4,), sent, dtype=dA.dtype, device="cuda")
    dU = torch.full((batch * su,), sent, dtype=dA.dtype, device="cuda")
    dV = torch.full((batch * sv,), sent, dtype=dA.dtype, device="cuda")
    dI = torch.full((batch + 2,), -9, dtype=torch.int32, device="cuda")
    S.lib.brd_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    fn = getattr(S.lib, f"brd_svd_batched_{sfx}")
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
        check_svd(dense[i].astype(np.float64), U[i], hS[i * n:(i + 1) * n], V[i], dtype)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_values_only_determinism_and_async(sfx):
    import torch
    dtype = DT[sfx]
    lim_s = 1e-13 if sfx == "f64" else 2e-5
    A = np.random.default_rng(51).uniform(0, 5, (7, 40, 24)).astype(dtype)
    dA = torch.from_numpy(A).cuda()
    U1, S1, Vh1 = S.svd_batched(dA)
    U2, S2, Vh2 = S.svd_batched(dA)
    for a, b in ((U1, U2), (S1, S2), (Vh1, Vh2)):
        assert torch.equal(a, b), "two identical calls differ"
    Sv = S.svdvals_batched(dA)
    assert Sv.shape == S1.shape
    err = (Sv - S1).abs().max(dim=1).values / S1[:, 0]
    assert float(err.max()) <= lim_s
    U3, S3, Vh3, info = S.svd_batched(dA, check=False, sync=False)
    torch.cuda.synchronize()
    assert torch.equal(U3, U1) and torch.equal(S3, S1) and torch.equal(Vh3, Vh1)
    assert int(info.abs().sum()) == 0
    # a single matrix: shaped like torch.linalg.svd(A, full_matrices=False)
    u, s, vh = S.svd_batched(dA[3])
    assert u.shape == (40, 24) and s.shape == (24,) and vh.shape == (24, 24)
    assert torch.equal(s, S1[3])


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_wide_input_through_the_transpose(sfx):
    dtype = DT[sfx]
    lim_r = 2e-13 if sfx == "f64" else 5e-5
    A = np.random.default_rng(61).uniform(0, 5, (3, 16, 40)).astype(dtype)
    U, Sv, Vh = _run(A)
    assert U.shape == (3, 16, 16) and Sv.shape == (3, 16) and Vh.shape == (3, 16, 40)
    for i in range(3):
        A64 = A[i].astype(np.float64)
        rec = (U[i].astype(np.float64) * Sv[i].astype(np.float64)) @ Vh[i].astype(np.float64)
        assert np.linalg.norm(rec - A64) <= lim_r * np.linalg.norm(A64)
        # the transposed problem passes every measure
        check_svd(A64.T, Vh[i].T, Sv[i], U[i], dtype)


@pytest.mark.parametrize("sfx,factor", [("f64", 1e150), ("f64", 1e-150), ("f32", 1e18), ("f32", 1e-18)])
def test_power_of_two_scaling_covers_the_range(sfx, factor):
    """Squares of these entries overflow / underflow; the kernel scales first."""
    dtype = DT[sfx]
    A = (np.random.default_rng(71).uniform(1, 2, (2, 20, 12)) * factor).astype(dtype)
    U, Sv, Vh, info = _run(A, check=False)
    assert np.array_equal(info, np.zeros(2, np.int32))
    _check_batch(A, U, Sv, Vh, dtype)


def test_graded_matrices_relative_accuracy(golden_dir):
    """A = B D with D over 2^-40 (fp64) / 2^-20 (fp32): every singular value to
    relative accuracy (the model: 3.1e-15 / 1.1e-6; measured on MI355X:
    2.6e-15 / 1.2e-6).  The two-stage route promises eps sigma_max only, so it
    cannot keep the small ones.  (Measured: on the zero-padded matrix it misses
    by far more than that -- it returns 1.199 for the three largest values,
    1.2 sigma_1 off, at every band width: DESIGN.md "Batched small SVD".)"""
    import torch
    g = np.load(os.path.join(golden_dir, "batched_graded.npz"))
    for sfx, lim in (("f64", 1e-13), ("f32", 2e-5)):
        A, ref = g[f"A_{sfx}"], g[f"S_{sfx}"]
        assert A.dtype == DT[sfx]
        Sv, info = _run(A, compute_uv=False, check=False)
        assert np.array_equal(info, np.zeros(A.shape[0], np.int32))
        rel = np.max(np.abs(Sv.astype(np.float64) - ref) / ref)
        print(f"graded {sfx}: worst relative error {rel:.2e}")
        assert rel <= lim
    # the contrast: singular_values_gpu on the first fp64 matrix, padded to
    # 24 x 24 with zero columns (same nonzero singular values)
    A0, ref0 = g["A_f64"][0], g["S_f64"][0]
    P = np.zeros((24, 24))
    P[:, :16] = A0
    two = S.singular_values_gpu(torch.from_numpy(P).cuda(), b=24).cpu().numpy()[:16]
    rel_small = abs(two[15] - ref0[15]) / ref0[15]
    print(f"two-stage route, smallest value: relative error {rel_small:.2e}, "
          f"absolute {np.max(np.abs(two - ref0)) / ref0[0]:.2e} sigma_1")
    assert rel_small > 1e-13


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_non_finite_matrix_is_flagged_and_isolated(sfx):
    dtype = DT[sfx]
    A = np.random.default_rng(81).uniform(0, 5, (5, 16, 16)).astype(dtype)
    A[2, 7, 3] = np.nan
    U, Sv, Vh, info = _run(A, check=False)
    assert info.tolist() == [0, 0, 2, 0, 0]
    assert np.all(np.isnan(U[2])) and np.all(np.isnan(Sv[2])) and np.all(np.isnan(Vh[2]))
    keep = [0, 1, 3, 4]
    _check_batch(A[keep], U[keep], Sv[keep], Vh[keep], dtype)
    # check=True leaves the NaNs in place and does not raise for info 2
    U2, S2, Vh2 = _run(A)
    assert np.all(np.isnan(S2[2])) and not np.any(np.isnan(S2[keep]))
    A[2, 7, 3] = np.inf
    assert _run(A, compute_uv=False, check=False)[1].tolist() == [0, 0, 2, 0, 0]


def test_profile_kind_and_size_limits():
    import torch
    A = torch.rand((4, 8, 8), dtype=torch.float64, device="cuda")
    S.profile_enable(True)
    S.profile_reset()
    S.svd_batched(A)
    q = S.profile_query("svd_batched")
    S.profile_enable(False)
    assert q["launches"] == 1 and q["ms"] > 0
    assert q["bytes"] == 4 * (64 + 8 + 64 + 64) * 8 + 4 * 4
    with pytest.raises(S.BrdError) as ei:
        S.svd_batched(torch.zeros((2, 129, 8), device="cuda"))
    assert ei.value.code == -5
