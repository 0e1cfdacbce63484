"""Batched least squares and pseudo-inverse on the GPU (brd_gelss_batched_*,
svdsolver_amd.lstsq_batched / pinv_batched): brd_gesvd_batched's launches, then
one launch that forms X = V diag(sigma+) (U^T B) from the factors.

Reference: numpy.linalg.lstsq / pinv / svd in float64 on the CPU, of the input
rounded to the dtype under test.  Limits, with lim = mid_model.mid_limits(n,
dtype) (values, reconstruction, orthogonality of the SVD factors) and tol =
lim[1] + lim[2] (ls_model.py):
    backward   |A^T (b - A x)| / (|A|_F^2 |x| + |A|_F |b|)            <= tol
    forward    |x - x_ref| <= tol kappa (1 + kappa |r| / (|A|_2 |x|)) |x|   (Wedin)
    rank       == n (full rank), == r (A = G1 G2 at an explicit rcond)
    null space |V0^T x| / |x|                                         <= lim[2]
    pinv       the four Penrose conditions <= tol, relative to |A|_F |P|_F
tests/test_ls_model.py shows that the numpy model of the method stays inside
them at every shape used here (its worst fraction of a limit: 0.0021).

Worst fractions of a limit measured on an MI355X (fp64 / fp32; the table in
DESIGN.md "Batched least squares" has them per check): backward 0.0005 /
0.0007, forward 0.0002 / 0.0002, null space 0.0023 / 0.0021, Penrose 0.0005 /
0.0009.
"""
import ctypes

import numpy as np
import pytest

import ls_model as M
import svdsolver_amd as S
from mid_model import mid_limits

pytestmark = pytest.mark.gpu

SFX = ["f64", "f32"]


def _ids(shapes):
    return ["x".join(str(v) for v in s) for s in shapes]


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _lstsq(A, B, rcond=None):
    """lstsq_batched on numpy batches; numpy (X, rank, S, info)."""
    return tuple(o.cpu().numpy() for o in S.lstsq_batched(_dev(A), _dev(B), rcond, check=False))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _f64(x):
    return x.astype(np.float64)


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("m,n,nrhs", M.LS_SHAPES + M.WIDE_SHAPES, ids=_ids(M.LS_SHAPES + M.WIDE_SHAPES))
def test_full_rank_against_numpy(m, n, nrhs, sfx):
    """Tall and square shapes, and wide ones (72 x 400, 3 x 5) through the transposed problem."""
    dtype = M.DT[sfx]
    A, B = (x.astype(dtype) for x in M.uniform_system(m, n, nrhs))
    X, rank, Sv, info = _lstsq(A, B)
    k = min(m, n)
    assert X.shape == (3, n, nrhs) and rank.shape == (3,) and Sv.shape == (3, k) and info.shape == (3,)
    assert X.dtype == dtype and Sv.dtype == dtype and rank.dtype == np.int32
    assert np.array_equal(info, np.zeros(3, np.int32))
    worst = np.zeros(2)
    for i in range(3):
        worst = np.maximum(worst, M.check_full_rank(_f64(A[i]), _f64(B[i]), X[i], rank[i], dtype))
    print(f"{m}x{n} nrhs {nrhs} {sfx}: backward {worst[0]:.4f} forward {worst[1]:.4f} of the limit")
    # S is the S of gesvd_batched with vectors, bit for bit
    assert _same_bits(Sv, S.gesvd_batched(_dev(A))[1].cpu().numpy())
    if nrhs == 1:   # the vector forms of B: (batch, m), and (m,) with a single matrix
        x1, r1, s1 = S.lstsq_batched(_dev(A), _dev(B[:, :, 0]))
        assert x1.shape == (3, n) and _same_bits(x1.cpu().numpy(), X[:, :, 0])
        x0, r0, s0 = S.lstsq_batched(_dev(A[1]), _dev(B[1, :, 0]))
        assert x0.shape == (n,) and r0.shape == () and s0.shape == (k,)
        assert _same_bits(x0.cpu().numpy(), X[1, :, 0]) and int(r0) == k


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("m,n,r", M.DEFICIENT, ids=_ids(M.DEFICIENT))
def test_rank_deficient_at_an_explicit_rcond(m, n, r, sfx):
    dtype = M.DT[sfx]
    A, B = (x.astype(dtype) for x in M.deficient_system(m, n, r))
    X, rank, Sv, info = _lstsq(A, B, M.DEFICIENT_RCOND[dtype])
    assert np.array_equal(info, np.zeros(3, np.int32))
    worst = np.zeros(2)
    for i in range(3):
        worst = np.maximum(worst, M.check_deficient(_f64(A[i]), _f64(B[i]), X[i], rank[i], r, dtype))
    print(f"{m}x{n} rank {r} {sfx}: null space {worst[0]:.4f} forward {worst[1]:.4f} of the limit")


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("m,n", M.PINV_SHAPES, ids=_ids(M.PINV_SHAPES))
def test_pinv_against_numpy(m, n, sfx):
    dtype = M.DT[sfx]
    A = M.uniform_system(m, n, 1)[0].astype(dtype)
    P = S.pinv_batched(_dev(A))
    assert tuple(P.shape) == (3, n, m)
    P = P.cpu().numpy()
    assert P.dtype == dtype
    worst = np.zeros(2)
    for i in range(3):
        worst = np.maximum(worst, M.check_pinv(_f64(A[i]), P[i], dtype))
    print(f"pinv {m}x{n} {sfx}: Penrose {worst[0]:.4f} distance {worst[1]:.4f} of the limit")
    # the identity as B gives the same matrix to the forward bound, and a single matrix is shaped (n, m)
    P1, info1 = S.pinv_batched(_dev(A[2]), check=False)
    assert tuple(P1.shape) == (n, m) and int(info1) == 0 and _same_bits(P1.cpu().numpy(), P[2])


@pytest.mark.parametrize("sfx", SFX)
def test_rcond_rules(sfx):
    dtype = M.DT[sfx]
    A, B = (x.astype(dtype) for x in M.uniform_system(300, 72, 17))
    A[1, :, 5] = 0                       # an exact zero singular value in matrix 1
    A[2] = 0                             # a zero matrix
    X, rank, Sv, info = _lstsq(A, B, 0.0)
    assert np.array_equal(info, np.zeros(3, np.int32))
    assert Sv[1, -1] == 0 and np.all(Sv[1, :-1] > 0)
    assert rank.tolist() == [72, 71, 0]  # rcond = 0 keeps every non-zero value
    assert np.all(X[2] == 0) and np.all(np.isfinite(X))
    A64 = _f64(np.delete(A[1], 5, axis=1))
    x_ref = np.linalg.lstsq(A64, _f64(B[1]), rcond=None)[0]
    assert np.all(X[1, 5] == 0)
    tol = M.tol_of(72, dtype)
    assert np.max(M.forward_fractions(A64, np.delete(X[1], 5, axis=0), _f64(B[1]), x_ref, tol)) <= 1
    for rc in (1.0, 3.0):                # sigma_j > rcond sigma_1 never holds
        X, rank, _, _ = _lstsq(A, B, rc)
        assert rank.tolist() == [0, 0, 0] and np.all(X == 0)
    X, rank, _, _ = _lstsq(A, B)         # the default: the zero matrix, and matrix 1's zero value dropped
    assert rank.tolist() == [72, 71, 0] and np.all(X[2] == 0)
    P = S.pinv_batched(_dev(A[2])).cpu().numpy()
    assert P.shape == (72, 300) and np.all(P == 0)


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("m,n,nrhs", [(300, 72, 17), (128, 64, 2), (72, 400, 17)],
                         ids=["300x72x17", "128x64x2", "72x400x17"])
def test_non_finite_matrix_is_flagged_and_isolated(m, n, nrhs, sfx):
    dtype = M.DT[sfx]
    A, B = (x.astype(dtype) for x in M.uniform_system(m, n, nrhs))
    clean = _lstsq(A, B)
    A[1, m // 2, 1] = np.nan
    X, rank, Sv, info = _lstsq(A, B)
    assert info.tolist() == [0, 2, 0]
    assert np.all(np.isnan(X[1])) and rank[1] == -1 and rank[0] == rank[2] == min(m, n)
    for got, ref in zip((X, Sv), (clean[0], clean[2])):
        assert _same_bits(got[[0, 2]], ref[[0, 2]]), "a neighbour changed"
    for i in (0, 2):
        M.check_full_rank(_f64(A[i]), _f64(B[i]), X[i], rank[i], dtype)
    P, pinfo = S.pinv_batched(_dev(A), check=False)
    assert pinfo.tolist() == [0, 2, 0] and bool(P[1].isnan().all()) and bool(P[[0, 2]].isfinite().all())
    # a non-finite B simply propagates, into its own column only
    B[0, 3, 0] = np.inf
    X2 = _lstsq(np.where(np.isfinite(A), A, 1).astype(dtype), B)[0]
    assert not np.any(np.isfinite(X2[0, :, 0])) and np.all(np.isfinite(X2[0, :, 1:])) and np.all(np.isfinite(X2[2]))


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("trans", [False, True], ids=["ls", "trans"])
def test_layout_padding_untouched_and_inputs_unchanged(trans, sfx):
    """The C ABI at 300 x 72 with nrhs = 17, lda = n + 3, ldb = nrhs + 2, ldx =
    nrhs + 1, padded batch strides, sentinels in all padding and 64 sentinel
    bytes behind work_bytes."""
    import torch
    dtype = M.DT[sfx]
    batch, m, n, nrhs = 4, 300, 72, 17
    rb, rx = (n, m) if trans else (m, n)          # rows of B and of X
    lda, ldb, ldx = n + 3, nrhs + 2, nrhs + 1
    sa, sb, sx = m * lda + 7, rb * ldb + 5, rx * ldx + 3
    sent = -777.0
    rng = np.random.default_rng(43)
    A = rng.uniform(0, 5, (batch, m, n)).astype(dtype)
    B = rng.uniform(-1, 1, (batch, rb, nrhs)).astype(dtype)

    def pack(dense, ld, stride):
        buf = np.full(batch * stride, sent, dtype=dtype)
        mask = np.zeros(batch * stride, dtype=bool)
        rows, cols = dense.shape[1:]
        for i in range(batch):
            for r in range(rows):
                o = i * stride + r * ld
                buf[o:o + cols] = dense[i, r]
                mask[o:o + cols] = True
        return buf, mask

    Abuf, _ = pack(A, lda, sa)
    Bbuf, _ = pack(B, ldb, sb)
    _, xmask = pack(np.zeros((batch, rx, nrhs), dtype), ldx, sx)
    dA, dB = _dev(Abuf), _dev(Bbuf)
    dX = torch.full((batch * sx,), sent, dtype=dA.dtype, device="cuda")
    dS = torch.full((batch * n + 4,), sent, dtype=dA.dtype, device="cuda")
    dR = torch.full((batch + 2,), -9, dtype=torch.int32, device="cuda")
    dI = torch.full((batch + 2,), -9, dtype=torch.int32, device="cuda")
    need = S.lib.brd_gelss_batched_work_bytes(batch, m, n, nrhs, A.itemsize)
    assert need > 0
    dW = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert dW.data_ptr() % 256 == 0
    S.lib.brd_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    fn = getattr(S.lib, f"brd_gelss_batched_{sfx}")
    rc = fn(dA.data_ptr(), batch, m, n, lda, sa, dB.data_ptr(), nrhs, ldb, sb, dX.data_ptr(), ldx, sx, -1.0,
            dS.data_ptr(), dR.data_ptr(), dI.data_ptr(), dW.data_ptr(), need, S.BRD_LS_TRANS if trans else 0)
    assert rc == 0, S.lib.brd_last_error()
    assert np.array_equal(dA.cpu().numpy().view(np.uint8), Abuf.view(np.uint8)), "A was written"
    assert np.array_equal(dB.cpu().numpy().view(np.uint8), Bbuf.view(np.uint8)), "B was written"
    assert np.all(dW.cpu().numpy()[need:] == 0xA5), "the workspace was written past work_bytes"
    hX, hS = dX.cpu().numpy(), dS.cpu().numpy()
    assert np.all(hX[~xmask] == sent), "padding of X was written"
    assert np.all(hS[batch * n:] == sent)
    assert dR.cpu().numpy().tolist() == [n] * batch + [-9, -9]
    assert dI.cpu().numpy().tolist() == [0] * batch + [-9, -9]
    for i in range(batch):
        X = np.array([hX[i * sx + r * ldx: i * sx + r * ldx + nrhs] for r in range(rx)])
        A64 = _f64(A[i]).T if trans else _f64(A[i])
        M.check_full_rank(A64, _f64(B[i]), X, n, dtype)
    # S and rank NULL, the identity as B: X is n x m (trans: m x n), nothing else is written
    cx = rb
    ldp = cx + 2
    sp = rx * ldp + 1
    dP = torch.full((batch * sp,), sent, dtype=dA.dtype, device="cuda")
    dW.fill_(0xA5)
    rc = fn(dA.data_ptr(), batch, m, n, lda, sa, None, -5, 0, 0, dP.data_ptr(), ldp, sp, -1.0, None, None,
            dI.data_ptr(), dW.data_ptr(), need, S.BRD_LS_TRANS if trans else 0)
    assert rc == 0, S.lib.brd_last_error()
    assert np.all(dW.cpu().numpy()[need:] == 0xA5), "the workspace was written past work_bytes"
    assert np.array_equal(dA.cpu().numpy().view(np.uint8), Abuf.view(np.uint8)), "A was written"
    hP = dP.cpu().numpy()
    pmask = np.zeros(batch * sp, dtype=bool)
    for i in range(batch):
        for r in range(rx):
            pmask[i * sp + r * ldp: i * sp + r * ldp + cx] = True
    assert np.all(hP[~pmask] == sent), "padding of the pseudo-inverse was written"
    for i in range(batch):
        P = np.array([hP[i * sp + r * ldp: i * sp + r * ldp + cx] for r in range(rx)])
        M.check_pinv(_f64(A[i]).T if trans else _f64(A[i]), P, dtype)


@pytest.mark.parametrize("sfx", SFX)
def test_two_calls_are_bit_identical(sfx):
    import torch
    rng = np.random.default_rng(53)
    dA = _dev(rng.uniform(0, 5, (5, 300, 97)).astype(M.DT[sfx]))
    dB = _dev(rng.uniform(-1, 1, (5, 300, 19)).astype(M.DT[sfx]))
    X1, r1, S1 = S.lstsq_batched(dA, dB)
    X2, r2, S2 = S.lstsq_batched(dA, dB)
    for a, b in ((X1, X2), (S1, S2), (r1, r2)):
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), "two calls differ"
    X3, r3, S3, info = S.lstsq_batched(dA, dB, check=False, sync=False)
    torch.cuda.synchronize()
    assert torch.equal(X3, X1) and torch.equal(S3, S1) and torch.equal(r3, r1) and int(info.abs().sum()) == 0
    # a right-hand side does not depend on its neighbours in the tile, nor a matrix on the batch
    X4 = S.lstsq_batched(dA[2], dB[2, :, 17:].contiguous())[0]
    assert torch.equal(X4, X1[2, :, 17:])
    P1, P2 = S.pinv_batched(dA), S.pinv_batched(dA)
    assert torch.equal(P1.view(torch.uint8), P2.view(torch.uint8))


@pytest.mark.parametrize("sfx", SFX)
def test_mixed_batch_each_matrix_against_its_own_reference(sfx):
    """300 different 200 x 72 systems with nrhs = 3 (more workgroups than CUs): batch indexing."""
    dtype = M.DT[sfx]
    rng = np.random.default_rng(33)
    A = rng.uniform(0, 5, (300, 200, 72))
    A *= rng.uniform(0.1, 10.0, (300, 1, 1))
    A[0] = 0.0
    A[299] = 0.0
    A[299, :72, :] = np.eye(72)
    A = A.astype(dtype)
    B = rng.uniform(-1, 1, (300, 200, 3)).astype(dtype)
    X, rank, Sv, info = _lstsq(A, B)
    assert np.array_equal(info, np.zeros(300, np.int32))
    assert rank[0] == 0 and np.all(X[0] == 0) and np.all(rank[1:] == 72)
    worst = np.zeros(2)
    for i in range(1, 300):
        worst = np.maximum(worst, M.check_full_rank(_f64(A[i]), _f64(B[i]), X[i], rank[i], dtype))
    print(f"mixed batch {sfx}: backward {worst[0]:.4f} forward {worst[1]:.4f} of the limit")
    assert np.max(np.abs(_f64(X[299]) - _f64(B[299, :72]))) <= mid_limits(72, dtype)[2]


def test_profile_kinds():
    import torch
    A = torch.rand((4, 300, 72), dtype=torch.float64, device="cuda")
    B = torch.rand((4, 300, 5), dtype=torch.float64, device="cuda")
    kinds = ("gelss_batched", "gelss_solve", "gesvd_batched", "svd_batched", "svd_mid_batched", "svd_tall_batched")
    S.profile_enable(True)
    S.profile_reset()
    S.lstsq_batched(A, B)
    q1 = {k: S.profile_query(k) for k in kinds}
    S.pinv_batched(A)
    q2 = {k: S.profile_query(k) for k in kinds}
    S.profile_enable(False)
    assert [q1[k]["launches"] for k in kinds] == [1, 1, 0, 0, 0, 0]
    assert [q2[k]["launches"] for k in kinds] == [2, 2, 0, 0, 0, 0]
    assert q1["gelss_batched"]["ms"] > q1["gelss_solve"]["ms"] > 0 and q1["gelss_solve"]["bytes"] == 0
    # A and B read, X and S written; then A read, the 72 x 300 pseudo-inverse and S written
    assert q1["gelss_batched"]["bytes"] == 4 * (300 * 72 + 300 * 5 + 72 * 5 + 72) * 8
    assert q2["gelss_batched"]["bytes"] - q1["gelss_batched"]["bytes"] == 4 * (300 * 72 + 72 * 300 + 72) * 8
    with pytest.raises(S.BrdError) as ei:
        S.lstsq_batched(torch.zeros((2, 300, 129), device="cuda"), torch.zeros((2, 300, 1), device="cuda"))
    assert ei.value.code == -5
