"""CPU-side checks of brd_gelss_batched_*: declared, exported, and every bad
argument is rejected before any GPU is touched (so this passes on a machine
without one).  The pointers are arbitrary non-null host addresses (the
workspace's a multiple of 256): no case here may get as far as looking at
them."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -5
LS_TRANS = 0x20
M, N, K = 300, 72, 5   # a valid request: 300 x 72, five right-hand sides


def test_symbols_declared_and_exported():
    import svdsolver_amd as S
    src = open(os.path.join(REPO, "include", "brd.h")).read()
    declared = set(re.findall(r"^\s*(?:int|long)\s*(brd_\w+)\s*\(", src, re.M))
    lib = ctypes.CDLL(S.LIB_PATH)
    for sym in ("brd_gelss_batched_f64", "brd_gelss_batched_f32", "brd_gelss_batched_work_bytes"):
        assert sym in declared
        assert sym in S.brd.EXPORTED
        assert hasattr(lib, sym)
    assert re.search(r"#define\s+BRD_LS_TRANS\s+0x20u", src) and S.BRD_LS_TRANS == LS_TRANS == S.brd.BRD_LS_TRANS
    for name in ("lstsq_batched", "pinv_batched"):
        assert callable(getattr(S, name)) and name in S.__all__


def query(batch, m, n, nrhs, elem):
    import svdsolver_amd as S
    return S.lib.brd_gelss_batched_work_bytes(batch, m, n, nrhs, elem)


def svd_query(batch, m, n, vectors, elem):
    import svdsolver_amd as S
    return S.lib.brd_gesvd_batched_work_bytes(batch, m, n, vectors, elem)


def call(sfx="f64", **over):
    """brd_gelss_batched_<sfx> on a valid 2 x (300 x 72), nrhs = 5 request with `over` applied."""
    import svdsolver_amd as S
    buf = np.zeros(4096, dtype=np.float64 if sfx == "f64" else np.float32)
    info = np.zeros(8, dtype=np.int32)
    p = buf.ctypes.data
    aligned = (p + 255) & ~255
    a = dict(A=p, batch=2, m=M, n=N, lda=N, stride_a=M * N, B=p, nrhs=K, ldb=K, stride_b=M * K, X=p, ldx=K,
             stride_x=N * K, rcond=-1.0, S=p, rank=info.ctypes.data, info=info.ctypes.data, work=aligned,
             work_bytes=None, flags=0)
    a.update(over)
    if a["work_bytes"] is None:
        a["work_bytes"] = max(query(2, max(a["m"], 1), min(max(a["n"], 1), 128), max(a["nrhs"], 1), buf.itemsize), 0)
    fn = getattr(S.lib, f"brd_gelss_batched_{sfx}")
    rc = fn(a["A"], a["batch"], a["m"], a["n"], a["lda"], a["stride_a"], a["B"], a["nrhs"], a["ldb"], a["stride_b"],
            a["X"], a["ldx"], a["stride_x"], a["rcond"], a["S"], a["rank"], a["info"], a["work"], a["work_bytes"],
            a["flags"])
    return rc, S.lib.brd_last_error()


# the words the message of each rejection must hold
BAD = {
    "null_A": (dict(A=None), b"NULL"),
    "null_info": (dict(info=None), b"NULL"),
    "batch_0": (dict(batch=0), b"batch"),
    "n_0": (dict(n=0, lda=N), b"n >= 1"),
    "m_lt_n": (dict(m=N - 1), b"m >= n"),
    "lda_small": (dict(lda=N - 1), b"lda"),
    "stride_a_small": (dict(stride_a=M * N - 1), b"stride_a"),
    "nrhs_0": (dict(nrhs=0), b"nrhs"),
    "ldb_small": (dict(ldb=K - 1), b"ldb"),
    "stride_b_small": (dict(stride_b=M * K - 1), b"stride_b"),
    "ldx_small": (dict(ldx=K - 1), b"ldx"),
    "stride_x_small": (dict(stride_x=N * K - 1), b"stride_x"),
    "null_X": (dict(X=None), b"X is NULL"),
    "null_work": (dict(work=None), b"work"),
    "work_unaligned": (dict(work=8 + (1 << 20)), b"256"),
    # the transposed problem: B is n x nrhs, X is m x nrhs
    "trans_stride_b_small": (dict(flags=LS_TRANS, stride_b=N * K - 1, stride_x=M * K), b"stride_b"),
    "trans_stride_x_small": (dict(flags=LS_TRANS, stride_b=N * K, stride_x=M * K - 1), b"stride_x"),
    # the identity: X is n x m, whatever nrhs says
    "pinv_ldx_small": (dict(B=None, nrhs=0, ldx=M - 1, stride_x=N * M), b"ldx"),
    "pinv_stride_x_small": (dict(B=None, nrhs=0, ldx=M, stride_x=N * M - 1), b"stride_x"),
    "pinv_trans_ldx_small": (dict(B=None, nrhs=0, flags=LS_TRANS, ldx=N - 1, stride_x=M * N), b"ldx"),
}


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_return_einval(case, sfx):
    over, word = BAD[case]
    rc, msg = call(sfx, **over)
    assert rc == EINVAL
    assert msg and b"brd_gelss_batched" in msg and word in msg


def test_s_and_rank_may_be_null_and_nrhs_is_ignored_without_b():
    """Such requests pass every argument check: what stops them here is the
    last one, that the (host) pointers are not device memory."""
    for over in (dict(S=None), dict(rank=None), dict(B=None, nrhs=-3, ldx=M, stride_x=N * M),
                 dict(B=None, nrhs=0, flags=LS_TRANS, ldx=N, stride_x=M * N),
                 dict(flags=LS_TRANS, stride_b=N * K, stride_x=M * K), dict(rcond=0.5)):
        rc, msg = call(**over)
        assert rc == EINVAL and b"device memory" in msg, msg


def test_order_of_the_checks():
    """gesvd_batched's checks first and in its order, then nrhs, ldb, ldx, X, work."""
    def word(**over):
        rc, msg = call(**over)
        assert rc in (EINVAL, EUNSUPPORTED)
        return rc, msg
    chain = [(dict(A=None), b"NULL"), (dict(batch=0), b"batch"), (dict(n=0), b"n >= 1"), (dict(m=N - 1), b"m >= n"),
             (dict(lda=N - 1), b"lda"), (dict(stride_a=0), b"stride_a"), (dict(nrhs=0), b"nrhs"),
             (dict(ldb=0), b"ldb"), (dict(ldx=0), b"ldx"), (dict(X=None), b"X is NULL"), (dict(work_bytes=0), b"work")]
    for i, (_, expect) in enumerate(chain):
        over = {}
        for o, _ in chain[i:]:   # this fault and every later one at once: the earliest is reported
            over.update(o)
        if "n" in over:
            over["lda"] = N - 1
        rc, msg = word(**over)
        assert expect in msg, (i, msg)
    # a bad argument on an oversize request is EINVAL; the size limit comes before the new checks
    assert call(n=130, lda=129, stride_a=M * 130)[0] == EINVAL
    rc, msg = call(n=130, lda=130, stride_a=M * 130, nrhs=0, X=None)
    assert rc == EUNSUPPORTED and b"128 columns" in msg


@pytest.mark.parametrize("sfx,elem", [("f64", 8), ("f32", 4)])
def test_work_bytes_one_short_is_einval(sfx, elem):
    need = query(2, M, N, K, elem)
    assert need > 0
    rc, msg = call(sfx, work_bytes=need - 1)
    assert rc == EINVAL and b"work_bytes" in msg
    assert call(sfx, work_bytes=0)[0] == EINVAL


def _r(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("elem", [8, 4])
@pytest.mark.parametrize("batch,m,n", [(1, 5, 3), (3, 128, 128), (4, 300, 33), (5, 300, 72), (7, 129, 65),
                                       (2, 4097, 128)])
def test_work_bytes_identity(batch, m, n, elem):
    """gesvd_batched's workspace with vectors, then U, V and S, every piece rounded up to 256 bytes."""
    w0 = svd_query(batch, m, n, 1, elem)
    assert w0 >= 0
    want = _r(w0) + _r(batch * m * n * elem) + _r(batch * n * n * elem) + _r(batch * n * elem)
    for nrhs in (1, 16, 1000):   # the solve keeps its tile on chip: nrhs does not enter
        assert query(batch, m, n, nrhs, elem) == want
    assert want % 256 == 0


def test_work_query_rejects_what_the_call_rejects():
    for bad in ((0, 300, 72, 1, 8), (4, 8, 72, 1, 8), (4, 300, 0, 1, 8), (4, 300, 72, 1, 2)):
        assert query(*bad) == EINVAL
    assert query(2, 300, 129, 1, 8) == EUNSUPPORTED
    rc, msg = call(n=129, lda=129, stride_a=M * 129, ldx=K, stride_x=129 * K)
    assert rc == EUNSUPPORTED and b"brd_gelss_batched" in msg


def test_python_wrappers_reject_host_arrays():
    import svdsolver_amd as S
    with pytest.raises(ValueError):
        S.lstsq_batched(np.zeros((2, 300, 72)), np.zeros((2, 300, 3)))
    with pytest.raises(ValueError):
        S.pinv_batched(np.zeros((2, 300, 72)))
