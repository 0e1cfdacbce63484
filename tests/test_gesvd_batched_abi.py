"""CPU-side checks of brd_gesvd_batched_*: declared, exported, and every bad
argument is rejected before any GPU is touched (so this passes on a machine
without one).  The pointers are arbitrary non-null host addresses: no case
here may get as far as looking at them."""
import ctypes
import os
import re

import numpy as np
import pytest

from tall_mid_model import RB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -5
M, N = 300, 72   # a valid request on the new route: three row blocks


def test_symbols_declared_and_exported():
    import svdsolver_amd as S
    src = open(os.path.join(REPO, "include", "brd.h")).read()
    declared = set(re.findall(r"^\s*(?:int|long)\s*(brd_\w+)\s*\(", src, re.M))
    lib = ctypes.CDLL(S.LIB_PATH)
    for sym in ("brd_gesvd_batched_f64", "brd_gesvd_batched_f32", "brd_gesvd_batched_work_bytes"):
        assert sym in declared
        assert sym in S.brd.EXPORTED
        assert hasattr(lib, sym)
    for name in ("gesvd_batched", "gesvdvals_batched"):
        assert callable(getattr(S, name)) and name in S.__all__


def query(batch, m, n, vectors, elem):
    import svdsolver_amd as S
    return S.lib.brd_gesvd_batched_work_bytes(batch, m, n, vectors, elem)


def tall_query(batch, m, n, vectors, elem):
    import svdsolver_amd as S
    return S.lib.brd_svd_tall_batched_work_bytes(batch, m, n, vectors, elem)


def call(sfx="f64", **over):
    """brd_gesvd_batched_<sfx> on a valid 2 x (300 x 72) request with `over` applied."""
    import svdsolver_amd as S
    buf = np.zeros(4096, dtype=np.float64 if sfx == "f64" else np.float32)
    info = np.zeros(8, dtype=np.int32)
    p = buf.ctypes.data
    a = dict(A=p, batch=2, m=M, n=N, lda=N, stride_a=M * N, S=p, U=p, ldu=N, stride_u=M * N, V=p, ldv=N,
             stride_v=N * N, info=info.ctypes.data, work=p, work_bytes=None, flags=0)
    a.update(over)
    if a["work_bytes"] is None:
        a["work_bytes"] = max(query(2, max(a["m"], 1), min(max(a["n"], 1), 128), 1, buf.itemsize), 0)
    fn = getattr(S.lib, f"brd_gesvd_batched_{sfx}")
    rc = fn(a["A"], a["batch"], a["m"], a["n"], a["lda"], a["stride_a"], a["S"], a["U"], a["ldu"], a["stride_u"],
            a["V"], a["ldv"], a["stride_v"], a["info"], a["work"], a["work_bytes"], a["flags"])
    return rc, S.lib.brd_last_error()


# the table of tests/test_svd_tall_batched_abi.py, on the 300 x 72 request
BAD = {
    "null_A": dict(A=None),
    "null_S": dict(S=None),
    "null_info": dict(info=None),
    "batch_0": dict(batch=0),
    "n_0": dict(n=0, lda=N),
    "m_lt_n": dict(m=N - 1),
    "lda_small": dict(lda=N - 1),
    "stride_a_small": dict(stride_a=M * N - 1),
    "ldu_small": dict(ldu=N - 1),
    "stride_u_small": dict(stride_u=M * N - 1),
    "ldv_small": dict(ldv=N - 1),
    "stride_v_small": dict(stride_v=N * N - 1),
    "only_U": dict(V=None),
    "only_V": dict(U=None),
    "null_work": dict(work=None),
}


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_return_einval(case, sfx):
    rc, msg = call(sfx, **BAD[case])
    assert rc == EINVAL
    assert msg and b"brd_gesvd_batched" in msg


@pytest.mark.parametrize("sfx,elem", [("f64", 8), ("f32", 4)])
@pytest.mark.parametrize("vectors", [1, 0])
def test_work_bytes_one_short_is_einval(sfx, elem, vectors):
    need = query(2, M, N, vectors, elem)
    assert need > 0
    over = {} if vectors else dict(U=None, V=None)
    rc, msg = call(sfx, work_bytes=need - 1, **over)
    assert rc == EINVAL and b"work_bytes" in msg
    assert call(sfx, work_bytes=0, **over)[0] == EINVAL


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_more_than_128_columns_is_eunsupported(sfx):
    n = 129
    rc, msg = call(sfx, n=n, lda=n, stride_a=M * n, ldu=n, stride_u=M * n, ldv=n, stride_v=n * n)
    assert rc == EUNSUPPORTED
    assert b"brd_gesvd_batched" in msg and b"128 columns" in msg
    assert query(2, M, n, 1, 8) == EUNSUPPORTED


def test_argument_errors_come_before_size_limits():
    """The order of the checks: a bad argument on an oversize request is EINVAL."""
    rc, _ = call(n=130, lda=129, stride_a=M * 130)
    assert rc == EINVAL


def test_work_query():
    for bad in ((0, 300, 72, 1, 8), (4, 8, 72, 1, 8), (4, 300, 0, 1, 8), (4, 300, 72, 1, 2)):
        assert query(*bad) == EINVAL
    # at most 128 rows: forwarded, nothing needed
    assert query(4, 128, 128, 1, 8) == 0 and query(4, 100, 37, 1, 8) == 0
    # at most 64 columns: the tall route's workspace
    for shape in ((4, 300, 16), (4, 129, 64)):
        for vectors in (1, 0):
            for elem in (8, 4):
                assert query(*shape, vectors, elem) == tall_query(*shape, vectors, elem) > 0
    # the new route: values only needs R alone; fp32 is half of fp64
    assert query(4, 300, 72, 0, 8) == 4 * 72 * 72 * 8
    assert query(4, 300, 72, 0, 4) == 4 * 72 * 72 * 4
    assert query(4, 300, 72, 1, 8) == 4 * (2 * 72 * 72 + 3 * 72) * 8
    assert query(4, 300, 72, 1, 4) * 2 == query(4, 300, 72, 1, 8)


@pytest.mark.parametrize("n", [65, 96, 128])
def test_row_block_of_the_model_is_the_library_s(n):
    """R, U_R and one scalar per column per row block: the query tells the block height."""
    def blocks(m):
        q = query(1, m, n, 1, 8)
        assert q % 8 == 0 and (q // 8 - 2 * n * n) % n == 0
        return (q // 8 - 2 * n * n) // n
    if RB > 128:   # at most 128 rows are forwarded and need no workspace
        assert blocks(RB) == 1
    else:
        assert query(1, RB, n, 1, 8) == 0
    assert blocks(RB + 1) == 2 and blocks(2 * RB) == 2 and blocks(2 * RB + 1) == 3


def test_python_wrapper_rejects_host_arrays():
    import svdsolver_amd as S
    with pytest.raises(ValueError):
        S.gesvd_batched(np.zeros((2, 300, 72)))
    with pytest.raises(ValueError):
        S.gesvdvals_batched(np.zeros((2, 300, 72)))
