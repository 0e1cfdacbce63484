"""Batched SVD behind one entry point on the GPU (brd_gesvd_batched_*,
svdsolver_amd.gesvd_batched): the three existing routes forwarded bitwise, and
the new one -- more than 128 rows with 65 to 128 columns: blocked Householder
QR in row blocks of 128, the mid-size Jacobi kernel on the R factors, U = Q U_R.

Reference: numpy.linalg.svd in float64 on the CPU, of the input rounded to the
dtype under test.  Limits (fp64 / fp32): mid_model.check_svd_mid's, i.e. those
of tests/test_gpu_svd_batched.py times n / 64; tests/test_tall_mid_model.py
shows that the numpy model of the method stays inside them at every shape used
here (worst measure of the model: 0.17 of its limit in fp64, 0.26 in fp32):
    max|S - S_ref|                <= 1e-13 / 2e-5 * n/64 * sigma_1
    |U S V^T - A|_F               <= 2e-13 / 5e-5 * n/64 * |A|_F
    |V^T V - I|_F, |U^T U - I|_F  <= 1e-12 / 5e-4 * n/64   (U: columns with
                                                     sigma_j > n eps sigma_1)
    graded golden set, values     <= 1e-13 / 2e-5 * n/64 relative
"""
import ctypes
import os

import numpy as np
import pytest

import svdsolver_amd as S
from mid_model import check_svd_mid, graded_limit, mid_limits
from tall_mid_model import GPU_SHAPES, uniform_batch

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}


def _run(A, fn=None, **kw):
    """gesvd_batched on a numpy batch; numpy results."""
    import torch
    out = (fn or S.gesvd_batched)(torch.from_numpy(np.ascontiguousarray(A)).cuda(), **kw)
    if isinstance(out, tuple):
        return tuple(o.cpu().numpy() for o in out)
    return out.cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check_batch(A, U, Sv, Vh, dtype):
    worst = np.zeros(4)
    for i in range(A.shape[0]):
        worst = np.maximum(worst, check_svd_mid(A[i].astype(np.float64), U[i], Sv[i], Vh[i].T, dtype))
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
    lim = mid_limits(n, dtype)
    frac = max(e[0] / lim[0], e[1] / lim[1], e[2] / lim[2], e[3] / lim[2])
    print(f"{m}x{n} {sfx}: values {e[0]:.2e} reconstruction {e[1]:.2e} V {e[2]:.2e} U {e[3]:.2e}; "
          f"worst fraction of a limit {frac:.2f}")
    # values only: the same R, the Jacobi kernel without V
    Sv2, info2 = _run(A, fn=S.gesvdvals_batched, check=False)
    assert np.array_equal(info2, info)
    assert np.max(np.abs(Sv2.astype(np.float64) - Sv) / Sv[:, :1]) <= lim[0]


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("m,n,name", [(100, 37, "svd_batched"), (128, 96, "svd_mid_batched"),
                                      (300, 33, "svd_tall_batched")])
def test_existing_routes_are_forwarded_bitwise(m, n, name, sfx):
    A = uniform_batch(m, n).astype(DT[sfx])
    got = _run(A, check=False)
    ref = _run(A, fn=getattr(S, name), check=False)
    assert len(got) == len(ref) == 4
    for a, b in zip(got, ref):
        assert _same_bits(a, b)
    vals = getattr(S, name.replace("svd_", "svdvals_", 1))
    for a, b in zip(_run(A, fn=S.gesvdvals_batched, check=False), _run(A, fn=vals, check=False)):
        assert _same_bits(a, b)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_wide_input_through_the_transpose(sfx):
    dtype = DT[sfx]
    A = np.random.default_rng(61).uniform(0, 5, (3, 72, 400)).astype(dtype)
    U, Sv, Vh = _run(A)
    assert U.shape == (3, 72, 72) and Sv.shape == (3, 72) and Vh.shape == (3, 72, 400)
    for i in range(3):
        check_svd_mid(A[i].astype(np.float64).T, Vh[i].T, Sv[i], U[i], dtype)


def _rank_deficient_72(rng):
    """rank_deficient_mid's pattern at 200 x 72: a duplicated column, a zero
    column and a combination of two others."""
    A = rng.uniform(0, 5, (200, 72))
    A[:, 70] = A[:, 2]
    A[:, 51] = 0.0
    A[:, 66] = 0.5 * A[:, 4] - 2.0 * A[:, 35]
    return A


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_mixed_batch_each_matrix_against_its_own_reference(sfx):
    """300 different 200 x 72 matrices (more workgroups than CUs): batch indexing."""
    dtype = DT[sfx]
    rng = np.random.default_rng(31)
    A = rng.uniform(0, 5, (300, 200, 72))
    A *= rng.uniform(0.1, 10.0, (300, 1, 1))
    A[0] = 0.0
    A[150] = _rank_deficient_72(rng)
    A[299] = 0.0
    A[299, :72, :] = np.eye(72)
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
    """The C ABI with lda = n + 3, batch stride m lda + 7, ldu = n + 1, ldv = n + 2
    (ldv > n in fp64: the memory-resident V of the Jacobi step), and a
    workspace with 64 sentinel bytes behind work_bytes."""
    import torch
    dtype = DT[sfx]
    batch, m, n = 5, 300, 72
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
    need = S.lib.brd_gesvd_batched_work_bytes(batch, m, n, 1, dense.itemsize)
    assert need == batch * (2 * n * n + 3 * n) * dense.itemsize
    dW = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    S.lib.brd_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    fn = getattr(S.lib, f"brd_gesvd_batched_{sfx}")
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
        check_svd_mid(dense[i].astype(np.float64), U[i], hS[i * n:(i + 1) * n], V[i], dtype)
    # values only: nothing but S and info is written, and R alone fits the smaller workspace
    need0 = S.lib.brd_gesvd_batched_work_bytes(batch, m, n, 0, dense.itemsize)
    assert need0 == batch * n * n * dense.itemsize
    dW.fill_(0xA5)
    dS2 = torch.full_like(dS, sent)
    dI.fill_(-9)
    rc = fn(dA.data_ptr(), batch, m, n, lda, sa, dS2.data_ptr(), None, 0, 0, None, 0, 0, dI.data_ptr(), dW.data_ptr(),
            need0, 0)
    assert rc == 0, S.lib.brd_last_error()
    assert np.all(dW.cpu().numpy()[need0:] == 0xA5), "the workspace was written past work_bytes"
    assert np.array_equal(dA.cpu().numpy().view(np.uint8), Abuf.view(np.uint8)), "A was written"
    assert np.array_equal(dI.cpu().numpy(), np.array([0] * batch + [-9, -9], np.int32))
    hS2 = dS2.cpu().numpy()
    assert np.all(hS2[batch * n:] == sent)
    lim_s = mid_limits(n, dtype)[0]
    for i in range(batch):
        a, b = hS2[i * n:(i + 1) * n].astype(np.float64), hS[i * n:(i + 1) * n].astype(np.float64)
        assert np.max(np.abs(a - b)) <= lim_s * b[0]


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_two_calls_are_bit_identical(sfx):
    import torch
    A = np.random.default_rng(51).uniform(0, 5, (5, 300, 97)).astype(DT[sfx])
    dA = torch.from_numpy(A).cuda()
    U1, S1, Vh1 = S.gesvd_batched(dA)
    U2, S2, Vh2 = S.gesvd_batched(dA)
    for a, b in ((U1, U2), (S1, S2), (Vh1, Vh2)):
        a, b = a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)
        assert torch.equal(a, b), "two identical calls differ"
    U3, S3, Vh3, info = S.gesvd_batched(dA, check=False, sync=False)
    torch.cuda.synchronize()
    assert torch.equal(U3, U1) and torch.equal(S3, S1) and torch.equal(Vh3, Vh1)
    assert int(info.abs().sum()) == 0
    # a single matrix: shaped like torch.linalg.svd(A, full_matrices=False)
    u, s, vh = S.gesvd_batched(dA[3])
    assert u.shape == (300, 97) and s.shape == (97,) and vh.shape == (97, 97)
    assert torch.equal(s, S1[3]) and torch.equal(u, U1[3]) and torch.equal(vh, Vh1[3])


@pytest.mark.parametrize("sfx,factor", [("f64", 1e150), ("f64", 1e-150), ("f32", 1e18), ("f32", 1e-18)])
def test_power_of_two_scaling_covers_the_range(sfx, factor):
    """Squares of these entries overflow / underflow; the factor kernel keeps a
    running power-of-two scale.  2^+-500 / 2^+-60 scales S exactly."""
    dtype = DT[sfx]
    A = np.random.default_rng(71).uniform(1, 2, (3, 300, 72)).astype(dtype)
    k = (500 if sfx == "f64" else 60) * (1 if factor > 1 else -1)
    S0 = _run(A)[1]
    U, Sv, Vh, info = _run(np.ldexp(A, k), check=False)
    assert np.array_equal(info, np.zeros(3, np.int32))
    assert np.array_equal(Sv, np.ldexp(S0, k)), "a power of two does not scale S exactly"
    As = (A.astype(np.float64) * factor).astype(dtype)
    U, Sv, Vh, info = _run(As, check=False)
    assert np.array_equal(info, np.zeros(3, np.int32))
    _check_batch(As, U, Sv, Vh, dtype)


# row 5 lies in the first row block (of 128 rows), row 200 in the second
@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("n,row", [(72, 5), (72, 200), (128, 5), (128, 200)])
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
    # Inf, values only
    A[2, row, 3] = np.inf
    Sv3, info3 = _run(A, fn=S.gesvdvals_batched, check=False)
    clean_vals = _run(np.where(np.isfinite(A), A, 1).astype(dtype), fn=S.gesvdvals_batched)
    assert info3.tolist() == [0, 0, 2, 0, 0] and np.all(np.isnan(Sv3[2]))
    assert _same_bits(Sv3[keep], clean_vals[keep])


def test_graded_matrices_relative_accuracy(golden_dir):
    """A = B D with cond(B) = 20 and D down to 2^-40 (fp64) / 2^-20 (fp32), two
    300 x 72 and one 257 x 128: every singular value to relative accuracy
    through the QR front end.  The working-precision numpy model reaches
    2.1e-14 / 9.7e-6 (0.11 / 0.24 of the limit)."""
    g = np.load(os.path.join(golden_dir, "batched_graded_tall_mid.npz"))
    for sfx in ("f64", "f32"):
        for i in range(3):
            A, ref = g[f"A_{sfx}_{i}"], g[f"S_{sfx}_{i}"]
            assert A.dtype == DT[sfx]
            Sv, info = _run(A[None], compute_uv=False, check=False)
            assert np.array_equal(info, np.zeros(1, np.int32))
            rel = np.max(np.abs(Sv[0].astype(np.float64) - ref) / ref)
            print(f"graded tall mid {sfx} {A.shape}: worst relative error {rel:.2e} "
                  f"(limit {graded_limit(A.shape[1], DT[sfx]):.2e})")
            assert rel <= graded_limit(A.shape[1], DT[sfx])


def test_profile_kind_and_size_limits():
    import torch
    A = torch.rand((4, 300, 72), dtype=torch.float64, device="cuda")
    S.profile_enable(True)
    S.profile_reset()
    S.gesvd_batched(A)
    q = S.profile_query("gesvd_batched")
    older = [S.profile_query(k) for k in ("svd_batched", "svd_mid_batched", "svd_tall_batched")]
    stages = [S.profile_query(k) for k in ("svd_tall_qr", "svd_tall_jacobi", "svd_tall_apply")]
    S.profile_enable(False)
    assert q["launches"] == 1 and q["ms"] > 0
    # A read, S, U, V and info written
    assert q["bytes"] == 4 * (300 * 72 + 72 + 300 * 72 + 72 * 72) * 8 + 4 * 4
    assert [o["launches"] for o in older] == [0, 0, 0]
    assert [s["launches"] for s in stages] == [1, 1, 1] and all(s["ms"] > 0 and s["bytes"] == 0 for s in stages)
    with pytest.raises(S.BrdError) as ei:
        S.gesvd_batched(torch.zeros((2, 300, 129), device="cuda"))
    assert ei.value.code == -5
