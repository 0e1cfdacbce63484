"""CPU-side checks of brd_svd_mid_batched_*: declared, exported, and every bad
argument is rejected before any GPU is touched (so this passes on a machine
without one).  The pointers are arbitrary non-null host addresses: the only
cases that get as far as looking at them are the ones that must pass the size
check, and those fail at the device-pointer check."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -5


def test_symbols_declared_and_exported():
    import svdsolver_amd as S
    src = open(os.path.join(REPO, "include", "brd.h")).read()
    declared = set(re.findall(r"^\s*int\s*(brd_\w+)\s*\(", src, re.M))
    lib = ctypes.CDLL(S.LIB_PATH)
    for sym in ("brd_svd_mid_batched_f64", "brd_svd_mid_batched_f32"):
        assert sym in declared
        assert sym in S.brd.EXPORTED
        assert hasattr(lib, sym)
        bound = getattr(S.lib, sym)
        assert bound.restype is ctypes.c_int
        assert list(bound.argtypes) == list(getattr(S.lib, sym.replace("_mid", "")).argtypes)
    assert callable(S.svd_mid_batched) and callable(S.svdvals_mid_batched)
    assert "svd_mid_batched" in S.__all__ and "svdvals_mid_batched" in S.__all__


def call(sfx="f64", name="brd_svd_mid_batched", **over):
    """<name>_<sfx> on a valid 2 x (6 x 4) request with `over` applied."""
    import svdsolver_amd as S
    buf = np.zeros(4096, dtype=np.float64 if sfx == "f64" else np.float32)
    info = np.zeros(8, dtype=np.int32)
    p = buf.ctypes.data
    a = dict(A=p, batch=2, m=6, n=4, lda=4, stride_a=24, S=p, U=p, ldu=4, stride_u=24, V=p, ldv=4, stride_v=16,
             info=info.ctypes.data, flags=0)
    a.update(over)
    fn = getattr(S.lib, f"{name}_{sfx}")
    rc = fn(a["A"], a["batch"], a["m"], a["n"], a["lda"], a["stride_a"], a["S"], a["U"], a["ldu"], a["stride_u"],
            a["V"], a["ldv"], a["stride_v"], a["info"], a["flags"])
    return rc, S.lib.brd_last_error()


def sized(m, n):
    return dict(m=m, n=n, lda=n, stride_a=m * n, ldu=n, stride_u=m * n, ldv=n, stride_v=n * n)


BAD = {
    "null_A": dict(A=None),
    "null_S": dict(S=None),
    "null_info": dict(info=None),
    "batch_0": dict(batch=0),
    "n_0": dict(n=0, lda=4),
    "m_lt_n": dict(m=3),
    "lda_small": dict(lda=3),
    "stride_a_small": dict(stride_a=23),
    "ldu_small": dict(ldu=3),
    "stride_u_small": dict(stride_u=23),
    "ldv_small": dict(ldv=3),
    "stride_v_small": dict(stride_v=15),
    "only_U": dict(V=None),
    "only_V": dict(U=None),
}


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_return_einval(case, sfx):
    rc, msg = call(sfx, **BAD[case])
    assert rc == EINVAL
    assert msg and b"brd_svd_mid_batched" in msg


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("m,n", [(129, 128), (200, 8)])
def test_size_limits_return_eunsupported(m, n, sfx):
    rc, msg = call(sfx, **sized(m, n))
    assert rc == EUNSUPPORTED
    assert b"128 x 128" in msg


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_m_less_than_n_is_einval(sfx):
    rc, msg = call(sfx, **sized(100, 128))
    assert rc == EINVAL and b"m >= n" in msg


def test_argument_errors_come_before_size_limits():
    """The order of the checks: a bad argument on an oversize request is EINVAL."""
    rc, _ = call(m=200, n=130, lda=129, stride_a=200 * 130)
    assert rc == EINVAL


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("m,n", [(128, 128), (65, 65)])
def test_sizes_within_the_limit_fail_only_at_the_device_pointer_check(m, n, sfx):
    buf = np.zeros(2 * m * n, dtype=np.float64 if sfx == "f64" else np.float32)
    rc, msg = call(sfx, A=buf.ctypes.data, S=buf.ctypes.data, U=buf.ctypes.data, V=buf.ctypes.data, **sized(m, n))
    assert rc == EINVAL
    assert b"device memory" in msg


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_svd_batched_keeps_its_limit(sfx):
    rc, msg = call(sfx, name="brd_svd_batched", **sized(65, 65))
    assert rc == EUNSUPPORTED
    assert b"128 x 64" in msg


def test_python_wrappers_reject_host_arrays():
    import svdsolver_amd as S
    with pytest.raises(ValueError):
        S.svd_mid_batched(np.zeros((2, 96, 96)))
    with pytest.raises(ValueError):
        S.svdvals_mid_batched(np.zeros((2, 96, 96)))
