"""Batched SVD of tall matrices on the GPU (brd_svd_tall_batched_*,
svdsolver_amd.svd_tall_batched): blocked Householder QR, the batched Jacobi
kernel on the R factors, U = Q U_R.

Reference: numpy.linalg.svd in float64 on the CPU, of the input rounded to the
dtype under test.  Limits (fp64 / fp32): those of tests/test_gpu_svd_batched.py,
unchanged; tests/test_tall_model.py shows that the numpy model of the method
stays inside them at every shape used here (worst measure of the model: 0.12
of its limit in fp64, 0.32 in fp32):
    max|S - S_ref|                <= 1e-13 / 2e-5 * sigma_1
    |U S V^T - A|_F               <= 2e-13 / 5e-5 * |A|_F
    |V^T V - I|_F, |U^T U - I|_F  <= 1e-12 / 5e-4   (U: columns with
                                                     sigma_j > n eps sigma_1)
    graded golden set, values     <= 1e-13 / 2e-5 relative
"""
import ctypes
import os

import numpy as np
import pytest

import svdsolver_amd as S
from jacobi_model import check_svd, rank_deficient
from tall_model import GPU_SHAPES, row_block, uniform_batch

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}


def _run(A, fn=None, **kw):
    """svd_tall_batched on a numpy batch; numpy results."""
    import torch
    out = (fn or S.svd_tall_batched)(torch.from_numpy(np.ascontiguousarray(A)).cuda(), **kw)
    if isinstance(out, tuple):
        return tuple(o.cpu().numpy() for o in out)
    return out.cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check_batch(A, U, Sv, Vh, dtype):
    worst = np.zeros(4)
    for i in range(A.shape[0]):
        worst = np.maximum(worst, check_svd(A[i].astype(np.float64), U[i], Sv[i], Vh[i].T, dtype))
    return worst


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("m,n", GPU_SHAPES, ids=[f"{m}x{n}" for m, n in GPU_SHAPES])
def test_shapes_against_numpy(m, n, sfx):
    dtype = DT[sfx]
    A = uniform_batch(m, n).astype(dtype)
    U, Sv, Vh, info = _run(A, check=False)
    assert U.shape == (3, m, n) and Sv.shape == (3, n) and Vh.shape == (3, n, n)
    assert U.dtype == dtype and Sv.dtype == dtype and Vh.dtype == dtype
    assert np.array_equal(info, np.zeros(3, np.int32))
    e = _check_batch(A, U, Sv, Vh, dtype)
    print(f"{m}x{n} {sfx} (row block {row_block(n)}): values {e[0]:.2e} reconstruction {e[1]:.2e} "
          f"V {e[2]:.2e} U {e[3]:.2e}")
    # values only: the same R, the Jacobi kernel without V
    Sv2, info2 = _run(A, fn=S.svdvals_tall_batched, check=False)
    assert np.array_equal(info2, info)
    lim_s = 1e-13 if sfx == "f64" else 2e-5
    assert np.max(np.abs(Sv2.astype(np.float64) - Sv) / Sv[:, :1]) <= lim_s


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("m,n", [(100, 37), (128, 64)])
def test_small_matrices_forward_to_svd_batched_bitwise(m, n, sfx):
    A = uniform_batch(m, n).astype(DT[sfx])
    tall = _run(A, check=False)
    small = _run(A, fn=S.svd_batched, check=False)
    for a, b in zip(tall, small):
        assert _same_bits(a, b)
    assert _same_bits(_run(A, fn=S.svdvals_tall_batched), _run(A, fn=S.svdvals_batched))


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_wide_input_through_the_transpose(sfx):
    dtype = DT[sfx]
    A = np.random.default_rng(61).uniform(0, 5, (3, 24, 500)).astype(dtype)
    U, Sv, Vh = _run(A)
    assert U.shape == (3, 24, 24) and Sv.shape == (3, 24) and Vh.shape == (3, 24, 500)
    for i in range(3):
        check_svd(A[i].astype(np.float64).T, Vh[i].T, Sv[i], U[i], dtype)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_mixed_batch_each_matrix_against_its_own_reference(sfx):
    """300 different 200 x 24 matrices (more workgroups than CUs): batch indexing."""
    dtype = DT[sfx]
    rng = np.random.default_rng(31)
    A = rng.uniform(0, 5, (300, 200, 24))
    A *= rng.uniform(0.1, 10.0, (300, 1, 1))
    A[0] = 0.0
    A[150] = rank_deficient(rng, 200, 24)
    A[299] = 0.0
    A[299, :24, :] = np.eye(24)
    A = A.astype(dtype)
    U, Sv, Vh, info = _run(A, check=False)
    assert np.array_equal(info, np.zeros(300, np.int32))
    _check_batch(A, U, Sv, Vh, dtype)
    assert np.all(Sv[0] == 0) and np.all(U[0] == 0)
    assert np.allclose(Sv[299], 1.0, rtol=0, atol=1e-6)
    # the zero column of the rank-deficient matrix: sigma = 0 and a zero column of U
    assert Sv[150, -1] == 0 and np.all(U[150, :, -1] == 0)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_layout_padding_untouched_and_input_unchanged(sfx):
    """The C ABI with lda = n + 3, batch stride m lda + 7, ldu = n + 1, ldv = n + 2,
    and a workspace with 64 sentinel bytes behind work_bytes."""
    import torch
    dtype = DT[sfx]
    batch, m, n = 5, 300, 12
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
    need = S.lib.brd_svd_tall_batched_work_bytes(batch, m, n, 1, dense.itemsize)
    assert need > 0
    dW = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    S.lib.brd_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    fn = getattr(S.lib, f"brd_svd_tall_batched_{sfx}")
    rc = fn(dA.data_ptr(), batch, m, n, lda, sa, dS.data_ptr(), dU.data_ptr(), ldu, su, dV.data_ptr(), ldv, sv,
            dI.data_ptr(), dW.data_ptr(), need, 0)
    assert rc == 0, S.lib.brd_last_error()
    assert np.array_equal(dA.cpu().numpy().view(np.uint8), Abuf.view(np.uint8)), "A was written"
    assert np.all(dW.cpu().numpy()[need:] == 0xA5), "the workspace was written past work_bytes"
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
    # values only: nothing but S and info is written, and R alone fits the smaller workspace
    need0 = S.lib.brd_svd_tall_batched_work_bytes(batch, m, n, 0, dense.itemsize)
    assert 0 < need0 < need
    dW.fill_(0xA5)
    dS2 = torch.full_like(dS, sent)
    rc = fn(dA.data_ptr(), batch, m, n, lda, sa, dS2.data_ptr(), None, 0, 0, None, 0, 0, dI.data_ptr(), dW.data_ptr(),
            need0, 0)
    assert rc == 0, S.lib.brd_last_error()
    assert np.all(dW.cpu().numpy()[need0:] == 0xA5), "the workspace was written past work_bytes"
    hS2 = dS2.cpu().numpy()
    assert np.all(hS2[batch * n:] == sent)
    lim_s = 1e-13 if sfx == "f64" else 2e-5
    for i in range(batch):
        a, b = hS2[i * n:(i + 1) * n].astype(np.float64), hS[i * n:(i + 1) * n].astype(np.float64)
        assert np.max(np.abs(a - b)) <= lim_s * b[0]


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_two_calls_are_bit_identical(sfx):
    import torch
    A = np.random.default_rng(51).uniform(0, 5, (5, 300, 33)).astype(DT[sfx])
    dA = torch.from_numpy(A).cuda()
    U1, S1, Vh1 = S.svd_tall_batched(dA)
    U2, S2, Vh2 = S.svd_tall_batched(dA)
    for a, b in ((U1, U2), (S1, S2), (Vh1, Vh2)):
        a, b = a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)
        assert torch.equal(a, b), "two identical calls differ"
    U3, S3, Vh3, info = S.svd_tall_batched(dA, check=False, sync=False)
    torch.cuda.synchronize()
    assert torch.equal(U3, U1) and torch.equal(S3, S1) and torch.equal(Vh3, Vh1)
    assert int(info.abs().sum()) == 0
    # a single matrix: shaped like torch.linalg.svd(A, full_matrices=False)
    u, s, vh = S.svd_tall_batched(dA[3])
    assert u.shape == (300, 33) and s.shape == (33,) and vh.shape == (33, 33)
    assert torch.equal(s, S1[3]) and torch.equal(u, U1[3])


@pytest.mark.parametrize("sfx,factor", [("f64", 1e150), ("f64", 1e-150), ("f32", 1e18), ("f32", 1e-18)])
def test_power_of_two_scaling_covers_the_range(sfx, factor):
    """Squares of these entries overflow / underflow; the factor kernel keeps a
    running power-of-two scale.  The factor's power-of-two part scales S exactly."""
    dtype = DT[sfx]
    A = np.random.default_rng(71).uniform(1, 2, (3, 300, 16)).astype(dtype)
    k = int(np.round(np.log2(factor)))
    S0 = _run(A)[1]
    U, Sv, Vh, info = _run(np.ldexp(A, k), check=False)
    assert np.array_equal(info, np.zeros(3, np.int32))
    assert np.array_equal(Sv, np.ldexp(S0, k)), "a power of two does not scale S exactly"
    As = (A.astype(np.float64) * factor).astype(dtype)
    U, Sv, Vh, info = _run(As, check=False)
    assert np.array_equal(info, np.zeros(3, np.int32))
    _check_batch(As, U, Sv, Vh, dtype)


# row 250 lies in the second row block of the 64-column class (blocks of 128)
# and in the first of the 16-column class (blocks of 256); row 290 is in the
# second block there too
@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("n,row", [(8, 250), (8, 290), (40, 250)])
def test_non_finite_matrix_is_flagged_and_isolated(n, row, sfx):
    dtype = DT[sfx]
    A = np.random.default_rng(81).uniform(0, 5, (5, 300, n)).astype(dtype)
    clean = _run(A, check=False)
    A[2, row, 3] = np.nan
    U, Sv, Vh, info = _run(A, check=False)
    assert info.tolist() == [0, 0, 2, 0, 0]
    assert np.all(np.isnan(U[2])) and np.all(np.isnan(Sv[2])) and np.all(np.isnan(Vh[2]))
    keep = [0, 1, 3, 4]
    for got, ref in zip((U, Sv, Vh), clean):
        assert _same_bits(got[keep], ref[keep]), "a neighbour changed"
    # check=True leaves the NaNs in place and does not raise for info 2
    S2 = _run(A)[1]
    assert np.all(np.isnan(S2[2])) and not np.any(np.isnan(S2[keep]))
    # Inf, values only
    A[2, row, 3] = np.inf
    Sv3, info3 = _run(A, fn=S.svdvals_tall_batched, check=False)
    clean_vals = _run(np.where(np.isfinite(A), A, 1).astype(dtype), fn=S.svdvals_tall_batched)
    assert info3.tolist() == [0, 0, 2, 0, 0] and np.all(np.isnan(Sv3[2]))
    assert _same_bits(Sv3[keep], clean_vals[keep])


def test_graded_matrices_relative_accuracy(golden_dir):
    """A = B D, 300 x 16, D over 2^-40 (fp64) / 2^-20 (fp32): every singular
    value to relative accuracy through the QR front end (the model: 2.5e-15 /
    7.1e-7)."""
    g = np.load(os.path.join(golden_dir, "batched_graded_tall.npz"))
    for sfx, lim in (("f64", 1e-13), ("f32", 2e-5)):
        A, ref = g[f"A_{sfx}"], g[f"S_{sfx}"]
        assert A.dtype == DT[sfx]
        Sv, info = _run(A, compute_uv=False, check=False)
        assert np.array_equal(info, np.zeros(A.shape[0], np.int32))
        rel = np.max(np.abs(Sv.astype(np.float64) - ref) / ref)
        print(f"graded tall {sfx}: worst relative error {rel:.2e}")
        assert rel <= lim


def test_profile_kind_and_size_limits():
    import torch
    A = torch.rand((4, 300, 8), dtype=torch.float64, device="cuda")
    S.profile_enable(True)
    S.profile_reset()
    S.svd_tall_batched(A)
    q = S.profile_query("svd_tall_batched")
    small = S.profile_query("svd_batched")
    S.profile_enable(False)
    assert q["launches"] == 1 and q["ms"] > 0
    # A read, S, U, V and info written
    assert q["bytes"] == 4 * (2400 + 8 + 2400 + 64) * 8 + 4 * 4
    assert small["launches"] == 0
    with pytest.raises(S.BrdError) as ei:
        S.svd_tall_batched(torch.zeros((2, 300, 65), device="cuda"))
    assert ei.value.code == -5
