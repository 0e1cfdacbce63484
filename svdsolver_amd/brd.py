"""Python host side of the MI355X two-stage bidiagonal reduction.

Mirrors the reference's operator interface for the hot path:

* :func:`brd_p1` / :func:`cuda_brd_p1` -- dense -> band, like
  ``csc586::gpu::cuda_brd_p1(Matrix<float>& A, size_t b)`` (reference
  svd_cuda_2.cu:1117) and ``csc586::parallel::brd_p1<T>`` (svd_parallel.h:411):
  takes an N x N matrix and the band width b, returns the band matrix.
* :func:`brd_p2` -- band -> bidiagonal with the reference's window geometry,
  like ``csc586::parallel::brd_p2<T>`` (svd_parallel.h:640): returns the
  matrix after the sweeps plus the ``Bidiagonal{d, e}`` vectors.

Every call goes through the C ABI of ``lib/libbrd_hip.so`` (include/brd.h).
numpy arrays take the host-pointer path (the library stages them through
HBM); torch CUDA tensors are reduced in place on the device, on torch's
current stream.  There is no CPU fallback: if the HIP library is missing the
import of this module fails.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# BRD_LIB: another build of the same library (developer A/B runs)
LIB_PATH = os.environ.get("BRD_LIB") or os.path.join(_HERE, "lib", "libbrd_hip.so")

BRD_DEVICE_PTR = 0x1
BRD_ASYNC = 0x2
BRD_COMPAT = 0x0
BRD_EXACT_ORDER = 0x4
BRD_NO_EXTRACT = 0x8
BRD_SIGMA = 0x10
BRD_LS_TRANS = 0x20

EXPORTED = (
    "brd_ge2band_f64", "brd_ge2band_f32", "brd_band2bd_f64", "brd_band2bd_f32",
    "brd_set_stream", "brd_use_own_stream", "brd_set_overlap", "brd_check_errors", "brd_release_stream", "brd_profile_enable", "brd_profile_reset", "brd_profile_query",
    "brd_dist_unique_id", "brd_dist_init", "brd_dist_init_host", "brd_dist_finalize", "brd_dist_local_cols",
    "brd_ge2band_dist_f64", "brd_ge2band_dist_f32", "brd_dist_gather_band_f64", "brd_dist_gather_band_f32",
    "brd_bdsvd_f64", "brd_bdsvd_f32", "brd_bdsvd_dev_f64", "brd_bdsvd_dev_f32", "brd_last_error", "brd_version",
    "brd_svd_batched_f64", "brd_svd_batched_f32", "brd_svd_mid_batched_f64", "brd_svd_mid_batched_f32",
    "brd_svd_tall_batched_work_bytes", "brd_svd_tall_batched_f64", "brd_svd_tall_batched_f32",
    "brd_gesvd_batched_work_bytes", "brd_gesvd_batched_f64", "brd_gesvd_batched_f32",
    "brd_gelss_batched_work_bytes", "brd_gelss_batched_f64", "brd_gelss_batched_f32",
)

# brd_coll_fn (include/brd.h): int (*)(int op, const void *send, void *recv,
#                                     unsigned long count, int dtype, int root, void *user)
COLL_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulong,
                           ctypes.c_int, ctypes.c_int, ctypes.c_void_p)


class BrdError(RuntimeError):
    """Raised when a libbrd_hip entry point returns a negative brd_status."""

    def __init__(self, fn: str, code: int, msg: str):
        super().__init__(f"{fn} failed ({code}): {msg}")
        self.code = code


def _load() -> ctypes.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C svdsolver_amd` "
            "(or __graft_entry__.build()); there is no CPU fallback")
    # torch bundles its own HIP runtime (torch/lib/libamdhip64.so, SONAME
    # libamdhip64.so.7).  Loaded after libbrd_hip.so (which needs
    # /opt/rocm's libamdhip64.so.7), torch would bring a second runtime that
    # does not know the library's device pointers and vice versa; loading
    # torch first lets the library bind to the runtime already in the process.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, ci, cu = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
    for t in ("f64", "f32"):
        f = getattr(L, f"brd_ge2band_{t}")
        f.argtypes = [vp, ci, ci, ci, ci, ci, cu]
        f.restype = ci
        g = getattr(L, f"brd_band2bd_{t}")
        g.argtypes = [vp, ci, ci, ci, vp, vp, cu]
        g.restype = ci
        h = getattr(L, f"brd_bdsvd_{t}")
        h.argtypes = [vp, vp, ci, vp]
        h.restype = ci
        hd = getattr(L, f"brd_bdsvd_dev_{t}")
        hd.argtypes = [vp, vp, ci, vp, cu]
        hd.restype = ci
        sb = getattr(L, f"brd_svd_batched_{t}")
        sb.argtypes = [vp, ci, ci, ci, ci, ctypes.c_long, vp, vp, ci, ctypes.c_long, vp, ci, ctypes.c_long, vp, cu]
        sb.restype = ci
        sm = getattr(L, f"brd_svd_mid_batched_{t}")
        sm.argtypes = list(sb.argtypes)
        sm.restype = ci
        st =getattr(L, f"brd_svd_tall_batched_{t}")
        st.argtypes = sb.argtypes[:-1] + [vp, ctypes.c_long, cu]
        st.restype = ci
        sg = getattr(L, f"brd_gesvd_batched_{t}")
        sg.argtypes = list(st.argtypes)
        sg.restype = ci
        ls = getattr(L, f"brd_gelss_batched_{t}")
        ls.argtypes = [vp, ci, ci, ci, ci, ctypes.c_long, vp, ci, ci, ctypes.c_long, vp, ci, ctypes.c_long,
                       ctypes.c_double if t == "f64" else ctypes.c_float, vp, vp, vp, vp, ctypes.c_long, cu]
        ls.restype = ci
    for q in (L.brd_svd_tall_batched_work_bytes, L.brd_gesvd_batched_work_bytes, L.brd_gelss_batched_work_bytes):
        q.argtypes = [ci, ci, ci, ci, ci]
        q.restype = ctypes.c_long
    L.brd_set_stream.argtypes = [vp]
    L.brd_set_stream.restype = ci
    L.brd_use_own_stream.argtypes = []
    L.brd_use_own_stream.restype = ci
    L.brd_set_overlap.argtypes = [ci]
    L.brd_set_overlap.restype = ci
    L.brd_check_errors.argtypes = []
    L.brd_check_errors.restype = ci
    L.brd_release_stream.argtypes = [ctypes.c_void_p]
    L.brd_release_stream.restype = ci
    L.brd_profile_enable.argtypes = [ci]
    L.brd_profile_enable.restype = ci
    L.brd_profile_reset.argtypes = []
    L.brd_profile_reset.restype = ci
    L.brd_profile_query.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_longlong),
                                    ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                    ctypes.POINTER(ctypes.c_double)]
    L.brd_profile_query.restype = ci
    L.brd_dist_unique_id.argtypes = [vp, ci]
    L.brd_dist_unique_id.restype = ci
    L.brd_dist_init.argtypes = [ci, ci, vp, ci]
    L.brd_dist_init.restype = ci
    L.brd_dist_init_host.argtypes = [ci, ci, COLL_FN, vp]
    L.brd_dist_init_host.restype = ci
    L.brd_dist_finalize.argtypes = []
    L.brd_dist_finalize.restype = ci
    L.brd_dist_local_cols.argtypes = [ci, ci, ci, ci]
    L.brd_dist_local_cols.restype = ci
    for t in ("f64", "f32"):
        f = getattr(L, f"brd_ge2band_dist_{t}")
        f.argtypes = [vp, ci, ci, ci, ci, cu]
        f.restype = ci
        g = getattr(L, f"brd_dist_gather_band_{t}")
        g.argtypes = [vp, ci, ci, ci, ci, vp, ci, ci, cu]
        g.restype = ci
    L.brd_last_error.argtypes = []
    L.brd_last_error.restype = ctypes.c_char_p
    L.brd_version.argtypes = []
    L.brd_version.restype = ci
    return L


lib = _load()


def _check(fn: str, rc: int) -> None:
    if rc != 0:
        raise BrdError(fn, rc, lib.brd_last_error().decode(errors="replace"))


def _sfx(dtype) -> str:
    s = str(dtype)
    if s in ("float64", "torch.float64"):
        return "f64"
    if s in ("float32", "torch.float32"):
        return "f32"
    raise TypeError(f"unsupported dtype {dtype} (float32 / float64 only)")


def _is_torch_cuda(x) -> bool:
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)


def _bind_stream(x) -> None:
    import torch
    lib.brd_set_stream(ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))


def _row_stride(A) -> int:
    """Leading dimension of a row-major CUDA tensor: contiguous rows
    (stride(1) == 1) at any row stride >= n (lda, as in the C ABI)."""
    m, n = A.shape
    if A.stride(1) != 1 or A.stride(0) < n:
        raise ValueError("A must be row-major with unit column stride and row stride >= n")
    return int(A.stride(0))


# ---------------------------------------------------------------------------
# stage 1
# ---------------------------------------------------------------------------
def ge2band(A, b: int, *, sync: bool = True):
    """Dense -> band (bandwidth ``b``) IN PLACE.  ``A`` is a C-contiguous
    float32/float64 numpy array (host path) or torch CUDA tensor (device
    path, torch's current stream).  Returns ``A``."""
    m, n = A.shape
    sfx = _sfx(A.dtype)
    fn = f"brd_ge2band_{sfx}"
    if _is_torch_cuda(A):
        lda = _row_stride(A)
        _bind_stream(A)
        flags = BRD_DEVICE_PTR | (0 if sync else BRD_ASYNC)
        _check(fn, getattr(lib, fn)(ctypes.c_void_p(A.data_ptr()), m, n, lda, int(b), 1, flags))
    else:
        if not (isinstance(A, np.ndarray) and A.flags.c_contiguous):
            raise TypeError("host path needs a C-contiguous numpy array")
        _check(fn, getattr(lib, fn)(ctypes.c_void_p(A.ctypes.data), m, n, n, int(b), 1, 0))
    return A


def brd_p1(A, b: int):
    """Reference-compatible dense -> band: returns the band matrix (a copy for
    numpy input, like ``csc586::parallel::brd_p1`` returning ``Matrix``)."""
    if _is_torch_cuda(A):
        return ge2band(A.contiguous().clone(), b)
    return ge2band(np.array(A, copy=True, order="C"), b)


cuda_brd_p1 = brd_p1   # name of the reference GPU entry point (svd_cuda_2.cu:1117)


# ---------------------------------------------------------------------------
# stage 2
# ---------------------------------------------------------------------------
def band2bd(A, b: int, *, exact_order: bool = False, sigma: bool = False, sync: bool = True,
            extract: bool = True):
    """Band -> bidiagonal IN PLACE with the reference's window geometry, or
    (``sigma``) the sigma-preserving one: the bidiagonal then has the band's
    singular values (BRD_SIGMA, include/brd.h).
    Returns (d, e) (None, None when ``extract`` is False)."""
    m, n = A.shape
    assert m == n, "stage 2 takes a square band matrix"
    sfx = _sfx(A.dtype)
    fn = f"brd_band2bd_{sfx}"
    flags = ((BRD_EXACT_ORDER if exact_order else 0) | (BRD_SIGMA if sigma else 0)
             | (0 if extract else BRD_NO_EXTRACT))
    if _is_torch_cuda(A):
        import torch
        _bind_stream(A)
        d = torch.empty(n, dtype=A.dtype, device=A.device) if extract else None
        e = torch.empty(max(n - 1, 1), dtype=A.dtype, device=A.device) if extract else None
        flags |= BRD_DEVICE_PTR | (0 if sync else BRD_ASYNC)
        _check(fn, getattr(lib, fn)(ctypes.c_void_p(A.data_ptr()), n, _row_stride(A), int(b),
                                    ctypes.c_void_p(d.data_ptr() if extract else 0),
                                    ctypes.c_void_p(e.data_ptr() if extract else 0), flags))
        return (d, e[: n - 1]) if extract else (None, None)
    if not (isinstance(A, np.ndarray) and A.flags.c_contiguous):
        raise TypeError("host path needs a C-contiguous numpy array")
    d = np.zeros(n, dtype=A.dtype)
    e = np.zeros(max(n - 1, 1), dtype=A.dtype)
    _check(fn, getattr(lib, fn)(ctypes.c_void_p(A.ctypes.data), n, n, int(b),
                                ctypes.c_void_p(d.ctypes.data), ctypes.c_void_p(e.ctypes.data), flags))
    return (d, e[: n - 1]) if extract else (None, None)


def brd_p2(A, b: int, *, exact_order: bool = False, sigma: bool = False) -> Tuple[object, object, object]:
    """Reference-compatible band -> bidiagonal: returns (A_after, d, e), where
    A_after is what the reference writes to bidiagonal_*.bin (``sigma``: the
    sigma-preserving variant, not in the reference)."""
    B = A.contiguous().clone() if _is_torch_cuda(A) else np.array(A, copy=True, order="C")
    d, e = band2bd(B, b, exact_order=exact_order, sigma=sigma)
    return B, d, e


# ---------------------------------------------------------------------------
# bidiagonal -> singular values (host), and the whole pipeline
# ---------------------------------------------------------------------------
def bdsvd(d, e):
    """Singular values (descending) of the upper bidiagonal (d, e) via the
    library's host Golub-Kahan QR (brd_bdsvd_*; replaces the reference's
    serial::qrd, svd_serial.h:368).  d, e: numpy arrays or torch tensors."""
    if _is_torch_cuda(d):
        d, e = d.cpu().numpy(), e.cpu().numpy()
    d = np.ascontiguousarray(d)
    e = np.ascontiguousarray(e, dtype=d.dtype)
    n = d.shape[0]
    if e.shape[0] != max(n - 1, 0):
        raise ValueError("e must have n - 1 entries")
    sfx = _sfx(d.dtype)
    sv = np.empty(n, dtype=d.dtype)
    ep = e if n > 1 else np.zeros(1, dtype=d.dtype)
    fn = f"brd_bdsvd_{sfx}"
    _check(fn, getattr(lib, fn)(ctypes.c_void_p(d.ctypes.data), ctypes.c_void_p(ep.ctypes.data), n,
                                ctypes.c_void_p(sv.ctypes.data)))
    return sv


def bdsvd_gpu(d, e, *, sync: bool = True):
    """Singular values (descending) of the upper bidiagonal (d, e) on the GPU:
    multisection on the Golub-Kahan tridiagonal, every value bracketed on its
    own (brd_bdsvd_dev_*; the host twin is :func:`bdsvd`).  d, e: torch CUDA
    tensors of one dtype (e has n - 1 entries); returns a CUDA tensor."""
    import torch
    if not (_is_torch_cuda(d) and (_is_torch_cuda(e) or d.shape[0] == 1)):
        raise ValueError("bdsvd_gpu takes torch CUDA tensors (use bdsvd for host arrays)")
    d = d.contiguous()
    n = d.shape[0]
    if e.shape[0] != max(n - 1, 0):
        raise ValueError("e must have n - 1 entries")
    e = e.to(d.dtype).contiguous()
    sfx = _sfx(d.dtype)
    sv = torch.empty_like(d)
    _bind_stream(d)
    fn = f"brd_bdsvd_dev_{sfx}"
    _check(fn, getattr(lib, fn)(ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(e.data_ptr() if n > 1 else 0), n,
                                ctypes.c_void_p(sv.data_ptr()), 0 if sync else BRD_ASYNC))
    return sv


def singular_values_gpu(A, b: int = 32):
    """Singular values of the square torch CUDA matrix A, every step on the GPU:
    stage 1, stage 2 with the sigma-preserving geometry, :func:`bdsvd_gpu`.
    A is not modified; returns a CUDA tensor (descending)."""
    M = A.clone()
    ge2band(M, b)
    d, e = band2bd(M, b, sigma=True)
    return bdsvd_gpu(d, e)


def singular_values(A, b: int = 32):
    """Singular values of the square matrix A: stage 1 (dense -> band, GPU),
    stage 2 with the sigma-preserving geometry (GPU), then bdsvd (host).
    A is not modified."""
    B = brd_p1(A, b)
    _, d, e = brd_p2(B, b, sigma=True)
    return bdsvd(d, e)


# ---------------------------------------------------------------------------
# batched SVD of small matrices (one-sided Jacobi, one launch)
# ---------------------------------------------------------------------------
def svd_batched(A, *, compute_uv: bool = True, check: bool = True, sync: bool = True):
    """SVD of a batch of small matrices in one kernel launch (brd_svd_batched_*,
    one-sided Jacobi; every matrix at most 128 x 64 or 64 x 128).  ``A`` is a
    float32/float64 torch CUDA tensor ``(batch, m, n)`` or ``(m, n)`` with
    contiguous rows (any row and batch stride); it is not modified.

    Returns ``(U, S, Vh)`` shaped like ``torch.linalg.svd(A,
    full_matrices=False)`` (``Vh`` is the transposed view of the library's V),
    or ``S`` alone when ``compute_uv`` is False.  Singular values are
    descending and relatively accurate for column-scaled matrices.

    ``check`` (implies a synchronise and one small copy): raise
    :class:`BrdError` naming the matrices that hit the sweep cap (info 1);
    matrices with a NaN or Inf (info 2) keep their all-NaN outputs, as torch
    does.  With ``check=False`` the per-matrix ``info`` tensor (int32) is
    returned as an extra last element and nothing is raised."""
    return _svd_batched_call(A, "svd_batched", None, compute_uv, check, sync)


def _svd_batched_call(A, name, work_query, compute_uv, check, sync):
    """The batched SVD entry points: argument rules, outputs and the call.
    ``work_query``: None, or (the name of the entry point's work-bytes query,
    its column limit) when the C ABI takes a caller-owned workspace."""
    import torch
    if not _is_torch_cuda(A):
        raise ValueError(f"{name} takes a torch CUDA tensor")
    if A.dim() not in (2, 3):
        raise ValueError("A must be (batch, m, n) or (m, n)")
    sfx = _sfx(A.dtype)
    single = A.dim() == 2
    A3 = A.unsqueeze(0) if single else A
    batch, m, n = A3.shape
    if batch < 1 or m < 1 or n < 1:
        raise ValueError(f"{name} needs batch, m, n >= 1")
    wide = m < n
    if wide:   # the C ABI keeps m >= n: decompose A^T = V S U^T
        A3 = A3.transpose(1, 2).contiguous()
        m, n = n, m
    if A3.stride(2) != 1 or A3.stride(1) < n or (batch > 1 and A3.stride(0) < (m - 1) * A3.stride(1) + n):
        raise ValueError("A must have unit column stride, row stride >= n and non-overlapping matrices")
    lda = int(A3.stride(1))
    stride_a = int(A3.stride(0)) if batch > 1 else m * lda
    S = torch.empty((batch, n), dtype=A.dtype, device=A.device)
    info = torch.empty(batch, dtype=torch.int32, device=A.device)
    U = V = None
    if compute_uv:
        U = torch.empty((batch, m, n), dtype=A.dtype, device=A.device)
        V = torch.empty((batch, n, n), dtype=A.dtype, device=A.device)
    work = ()
    if work_query:   # the caller-owned workspace of the C ABI: a tensor that lives until the call has run
        query, limit = work_query
        need = int(getattr(lib, query)(batch, m, n, int(compute_uv), A.element_size()))
        if need < 0:
            raise BrdError(query, need, f"{m} x {n} matrices are not supported "
                           f"(at most {limit} columns, or {limit} rows for wide input)")
        wbuf = torch.empty(max(need, 1), dtype=torch.uint8, device=A.device)
        work = (ctypes.c_void_p(wbuf.data_ptr() if need else 0), need)
    _bind_stream(A)
    fn = f"brd_{name}_{sfx}"
    wait = sync or check
    _check(fn, getattr(lib, fn)(ctypes.c_void_p(A3.data_ptr()), batch, m, n, lda, stride_a,
                                ctypes.c_void_p(S.data_ptr()),
                                ctypes.c_void_p(U.data_ptr() if compute_uv else 0), n, m * n,
                                ctypes.c_void_p(V.data_ptr() if compute_uv else 0), n, n * n,
                                ctypes.c_void_p(info.data_ptr()), *work, 0 if wait else BRD_ASYNC))
    if check:
        capped = torch.nonzero(info == 1).flatten().tolist()
        if capped:
            raise BrdError(fn, 1, f"sweep cap reached for matrices {capped}")
    if single:
        S, info = S[0], info[0]
        if compute_uv:
            U, V = U[0], V[0]
    if not compute_uv:
        return S if check else (S, info)
    # A = U S V^T; a wide input was decomposed as A^T = U S V^T, so A = V S U^T
    out = (V, S, U.transpose(-2, -1)) if wide else (U, S, V.transpose(-2, -1))
    return out if check else out + (info,)


def svdvals_batched(A, **kw):
    """Singular values only: ``svd_batched(A, compute_uv=False, **kw)``."""
    return svd_batched(A, compute_uv=False, **kw)


def svd_mid_batched(A, *, compute_uv: bool = True, check: bool = True, sync: bool = True):
    """SVD of a batch of matrices of at most 128 x 128 in one kernel launch
    (brd_svd_mid_batched_*, one-sided Jacobi, one workgroup per matrix).
    Matrices with at most 64 columns (or rows, for wide input) go to
    :func:`svd_batched`'s kernel unchanged; larger sizes raise
    :class:`BrdError` (code -5).

    Arguments, return values, ``check`` and ``sync`` are those of
    :func:`svd_batched`."""
    return _svd_batched_call(A, "svd_mid_batched", None, compute_uv, check, sync)


def svdvals_mid_batched(A, **kw):
    """Singular values only: ``svd_mid_batched(A, compute_uv=False, **kw)``."""
    return svd_mid_batched(A, compute_uv=False, **kw)


def svd_tall_batched(A, *, compute_uv: bool = True, check: bool = True, sync: bool = True):
    """SVD of a batch of tall matrices (brd_svd_tall_batched_*): any number of
    rows, at most 64 columns (or the transpose of that).  Blocked Householder
    QR of every matrix, :func:`svd_batched`'s Jacobi kernel on the n x n
    factors, then U = Q U_R -- three launches, no host synchronisation between
    them; relative accuracy for column-scaled matrices is kept.  Matrices of at
    most 128 rows go to :func:`svd_batched`'s kernel unchanged.

    Arguments, return values, ``check`` and ``sync`` are those of
    :func:`svd_batched`.  The workspace the C ABI asks for is allocated here as
    a torch tensor of the queried size."""
    return _svd_batched_call(A, "svd_tall_batched", ("brd_svd_tall_batched_work_bytes", 64), compute_uv, check, sync)


def svdvals_tall_batched(A, **kw):
    """Singular values only: ``svd_tall_batched(A, compute_uv=False, **kw)``."""
    return svd_tall_batched(A, compute_uv=False, **kw)


def gesvd_batched(A, *, compute_uv: bool = True, check: bool = True, sync: bool = True):
    """SVD of a batch of matrices of any number of rows and at most 128 columns
    (or the transpose of that) behind one call (brd_gesvd_batched_*).  The
    library picks the route by size: :func:`svd_batched`'s, :func:`svd_mid_batched`'s
    or :func:`svd_tall_batched`'s kernels (bitwise their results), and beyond
    128 rows with 65 to 128 columns a blocked Householder QR, the mid-size
    Jacobi kernel on the n x n factors and U = Q U_R.  More than 128 rows and
    columns raise :class:`BrdError` (code -5).

    Arguments, return values, ``check`` and ``sync`` are those of
    :func:`svd_batched`.  The workspace the C ABI asks for is allocated here as
    a torch tensor of the queried size."""
    return _svd_batched_call(A, "gesvd_batched", ("brd_gesvd_batched_work_bytes", 128), compute_uv, check, sync)


def gesvdvals_batched(A, **kw):
    """Singular values only: ``gesvd_batched(A, compute_uv=False, **kw)``."""
    return gesvd_batched(A, compute_uv=False, **kw)


# ---------------------------------------------------------------------------
# batched least squares and pseudo-inverse from the batched SVD factors
# ---------------------------------------------------------------------------
def _gelss_batched_call(A, B, name, rcond, check, sync):
    """brd_gelss_batched_*: the argument rules of :func:`_svd_batched_call` for
    ``A`` (and ``B``), the outputs and the call.  ``B`` None: the identity.
    Returns (X, rank, S, info), all with the batch dimension."""
    import torch
    if not _is_torch_cuda(A) or not (B is None or _is_torch_cuda(B)):
        raise ValueError(f"{name} takes torch CUDA tensors")
    if A.dim() not in (2, 3):
        raise ValueError("A must be (batch, m, n) or (m, n)")
    sfx = _sfx(A.dtype)
    A3 = A.unsqueeze(0) if A.dim() == 2 else A
    batch, m, n = A3.shape
    if batch < 1 or m < 1 or n < 1:
        raise ValueError(f"{name} needs batch, m, n >= 1")
    rows_b, rows_x = m, n
    flags = 0
    if m < n:   # the C ABI keeps m >= n: A x = b is (A^T)^T x = b
        A3 = A3.transpose(1, 2).contiguous()
        m, n = n, m
        flags |= BRD_LS_TRANS
    if A3.stride(2) != 1 or A3.stride(1) < n or (batch > 1 and A3.stride(0) < (m - 1) * A3.stride(1) + n):
        raise ValueError("A must have unit column stride, row stride >= n and non-overlapping matrices")
    lda = int(A3.stride(1))
    stride_a = int(A3.stride(0)) if batch > 1 else m * lda
    if B is None:
        nrhs, bptr, ldb, stride_b = rows_b, 0, 0, 0
    else:
        if B.dtype != A.dtype or B.device != A.device:
            raise ValueError("B must have A's dtype and device")
        if B.dim() != 3 or B.shape[0] != batch or B.shape[1] != rows_b or B.shape[2] < 1:
            raise ValueError(f"B must hold {rows_b} rows per matrix of A")
        nrhs = int(B.shape[2])
        if B.stride(2) != 1 or B.stride(1) < nrhs or (batch > 1 and B.stride(0) < (rows_b - 1) * B.stride(1) + nrhs):
            raise ValueError("B must have unit column stride, row stride >= its columns and non-overlapping matrices")
        ldb = int(B.stride(1))
        stride_b = int(B.stride(0)) if batch > 1 else rows_b * ldb
        bptr = B.data_ptr()
    need = int(lib.brd_gelss_batched_work_bytes(batch, m, n, nrhs, A.element_size()))
    if need < 0:
        raise BrdError("brd_gelss_batched_work_bytes", need, f"{m} x {n} matrices are not supported "
                       "(at most 128 columns, or 128 rows for wide input)")
    X = torch.empty((batch, rows_x, nrhs), dtype=A.dtype, device=A.device)
    S = torch.empty((batch, n), dtype=A.dtype, device=A.device)
    rank = torch.empty(batch, dtype=torch.int32, device=A.device)
    info = torch.empty(batch, dtype=torch.int32, device=A.device)
    wbuf = torch.empty(need, dtype=torch.uint8, device=A.device)   # lives until the call has run
    _bind_stream(A)
    fn = f"brd_gelss_batched_{sfx}"
    wait = sync or check
    _check(fn, getattr(lib, fn)(ctypes.c_void_p(A3.data_ptr()), batch, m, n, lda, stride_a,
                                ctypes.c_void_p(bptr), nrhs, ldb, stride_b,
                                ctypes.c_void_p(X.data_ptr()), nrhs, rows_x * nrhs,
                                -1.0 if rcond is None else float(rcond),
                                ctypes.c_void_p(S.data_ptr()), ctypes.c_void_p(rank.data_ptr()),
                                ctypes.c_void_p(info.data_ptr()), ctypes.c_void_p(wbuf.data_ptr()), need,
                                flags | (0 if wait else BRD_ASYNC)))
    if check:
        capped = torch.nonzero(info == 1).flatten().tolist()
        if capped:
            raise BrdError(fn, 1, f"sweep cap reached for matrices {capped}")
    return X, rank, S, info


def lstsq_batched(A, B, rcond=None, *, check: bool = True, sync: bool = True):
    """Minimum-norm least-squares solutions of a batch of systems through the
    batched SVD (brd_gelss_batched_*: :func:`gesvd_batched`'s launches and one
    more that forms ``V diag(1/s) U^T B`` without writing the factors' products
    to memory).  ``A`` is ``(batch, m, n)`` or ``(m, n)``, any number of rows
    and at most 128 columns or the transpose of that; ``B`` is ``(batch, m,
    k)`` or ``(batch, m)`` (``(m, k)`` or ``(m,)`` for a single matrix), both
    float32/float64 torch CUDA tensors with contiguous rows; neither is
    modified.

    Singular values ``s_j <= rcond * s_1`` are treated as zero (``rcond``
    None: ``max(m, n) * eps``, numpy's and torch's default).  Returns ``(X,
    rank, S)``: ``X`` shaped like ``B`` with n rows, ``rank`` (int32) the
    number of singular values kept per matrix, ``S`` the singular values
    (descending).  A matrix holding a NaN or Inf gets NaN and rank -1.

    ``check`` and ``sync`` are those of :func:`svd_batched`; with
    ``check=False`` the per-matrix ``info`` tensor is appended."""
    if not _is_torch_cuda(A) or not _is_torch_cuda(B):
        raise ValueError("lstsq_batched takes torch CUDA tensors")
    single = A.dim() == 2
    vec = B.dim() == (1 if single else 2)
    if B.dim() != A.dim() - (1 if vec else 0):
        raise ValueError("B must be (batch, m, k) or (batch, m) for a batch, (m, k) or (m,) for one matrix")
    B3 = B.unsqueeze(-1) if vec else B
    B3 = B3.unsqueeze(0) if single else B3
    X, rank, S, info = _gelss_batched_call(A, B3, "lstsq_batched", rcond, check, sync)
    if vec:
        X = X[..., 0]
    if single:
        X, rank, S, info = X[0], rank[0], S[0], info[0]
    return (X, rank, S) if check else (X, rank, S, info)


def pinv_batched(A, rcond=None, *, check: bool = True, sync: bool = True):
    """Pseudo-inverses of a batch of matrices through the batched SVD
    (brd_gelss_batched_* with the identity as right-hand side): ``A`` as for
    :func:`lstsq_batched`; returns ``P`` of shape ``(batch, n, m)`` (or ``(n,
    m)``) for either orientation, singular values ``s_j <= rcond * s_1``
    treated as zero.  ``check=False`` appends the ``info`` tensor."""
    X, _, _, info = _gelss_batched_call(A, None, "pinv_batched", rcond, check, sync)
    if _is_torch_cuda(A) and A.dim() == 2:
        X, info = X[0], info[0]
    return X if check else (X, info)


# ---------------------------------------------------------------------------
# stream of reductions: stage 2 of one matrix beside stage 1 of the next
# ---------------------------------------------------------------------------
def set_overlap(s2_cus: int) -> None:
    """brd_set_overlap (include/brd.h): run stage-2 sweeps on ``s2_cus``
    workgroups and size stage-1 launches for the remaining CUs, so that a
    band2bd on one stream and a ge2band on another share the chip; 0 restores
    the whole-chip defaults."""
    _check("brd_set_overlap", lib.brd_set_overlap(int(s2_cus)))


def overlap_cus(n: int) -> int:
    """CUs reserved for stage 2 when it overlaps stage 1.  Measured on MI355X
    (profiles/README.md, pipelined bench at n = 8192): 32 workgroups keep the
    sweep chain within 1 % of its whole-chip time and leave 224 CUs (28 per
    XCD) to stage 1 (93.7 ms beside the sweep, 88 ms alone); 64 gave 101.7 ms,
    and 40-56 or 72-128 were slower still (fp32: 16 and 24 slower than 32 too;
    the good values are multiples of 32, see profiles/README.md).  Stage 1
    dominates at larger n, so the reservation stays at 32."""
    return 32 if n >= 1024 else 16


def reduce_many(mats, b: int, *, sigma: bool = False, s2_cus: Optional[int] = None, sync: bool = True,
                lanes: int = 1, s2_lanes: Optional[int] = None):
    """Two-stage reduction of a sequence of square CUDA tensors, each in place,
    pipelined over pairs of HIP streams ("lanes"): on a lane, stage 2 of
    matrix i (its own stream, ``s2_cus`` workgroups) runs beside stage 1 of the
    lane's next matrix (the other stream, sized for the remaining CUs); matrix
    i goes to lane i mod ``lanes``.  Returns [(d, e)] per matrix (device
    tensors).  Each matrix sees exactly the calls of ge2band + band2bd; only
    their overlap differs.  The library's overlap setting is restored on exit.
    More than one lane pays only with one hardware queue per stream: set
    GPU_MAX_HW_QUEUES >= lanes + s2_lanes + 4 (at most 32) before HIP
    initialises ("lanes").  ``s2_lanes``: stage-2 streams (matrix
    i's stage 2 on stream i mod s2_lanes; default one per lane): fewer than
    the lanes make a burst of finished stage 1s queue for the sweep instead of
    each taking ``s2_cus`` CUs at once (bench.py: 10 lanes, 5 stage-2 streams).
    """
    import torch
    if not mats:
        return []
    if lanes < 1:
        raise ValueError("lanes must be >= 1")
    dev = mats[0].device
    cus = overlap_cus(mats[0].shape[0]) if s2_cus is None else int(s2_cus)
    lanes = min(int(lanes), len(mats))
    s2l = lanes if s2_lanes is None else max(1, min(int(s2_lanes), len(mats)))
    # every lane's stage-2 kernel is a persistent grid of ``cus`` workgroups,
    # one per CU (its LDS ring takes the CU), whose bundles wait on each
    # other: with more workgroups in flight than the chip holds, a partly
    # resident grid stalls ("Overlap and lanes")
    dev_cus = torch.cuda.get_device_properties(dev).multi_processor_count
    if s2l * cus > dev_cus:
        raise ValueError(f"stage-2 streams * s2_cus = {s2l} * {cus} exceeds the device's {dev_cus} CUs "
                         "(stage-2 grids must fit the chip together)")
    s_a = [torch.cuda.Stream(dev) for _ in range(lanes)]
    s_b = [torch.cuda.Stream(dev) for _ in range(s2l)]
    for s in s_a:
        s.wait_stream(torch.cuda.current_stream(dev))
    out = []
    set_overlap(cus)
    try:
        for i, A in enumerate(mats):
            sa, sb = s_a[i % lanes], s_b[i % s2l]
            with torch.cuda.stream(sa):
                ge2band(A, b, sync=False)
                done1 = torch.cuda.Event()
                done1.record(sa)
            with torch.cuda.stream(sb):
                sb.wait_event(done1)
                out.append(band2bd(A, b, sigma=sigma, sync=False))
    finally:
        set_overlap(0)
    for s in s_b:
        torch.cuda.current_stream(dev).wait_stream(s)
    if sync:
        torch.cuda.synchronize(dev)
        check_errors()
    return out


def release_stream(stream=None) -> None:
    """brd_release_stream (include/brd.h): drain ``stream`` (a torch CUDA
    stream; None: the library's current stream) and free the library's
    per-stream workspaces, staging buffer and error word; call before the
    stream is destroyed."""
    h = None if stream is None else ctypes.c_void_p(stream.cuda_stream)
    _check("brd_release_stream", lib.brd_release_stream(h))


def check_errors() -> None:
    """brd_check_errors (include/brd.h): drain the library's streams and raise
    :class:`BrdError` if an asynchronous stage-2 sweep hit its spin limit (its
    output is invalid) or a HIP error is pending."""
    _check("brd_check_errors", lib.brd_check_errors())


# ---------------------------------------------------------------------------
# profiling (per-kernel HIP-event timing inside the library)
# ---------------------------------------------------------------------------
def profile_enable(on: bool = True) -> None:
    _check("brd_profile_enable", lib.brd_profile_enable(1 if on else 0))


def profile_reset() -> None:
    _check("brd_profile_reset", lib.brd_profile_reset())


def profile_query(kernel: str) -> dict:
    n = ctypes.c_longlong()
    ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    _check("brd_profile_query", lib.brd_profile_query(kernel.encode(), ctypes.byref(n), ctypes.byref(ms),
                                                      ctypes.byref(fl), ctypes.byref(by)))
    return {"launches": n.value, "ms": ms.value, "flops": fl.value, "bytes": by.value}
