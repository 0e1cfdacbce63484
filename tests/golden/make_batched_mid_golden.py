"""Generator of tests/golden/batched_graded_mid.npz: graded matrices with 65
to 128 columns whose small singular values only a relatively accurate method
gets right.

Three matrices A = B D per dtype: 128 x 128, 100 x 72 and 128 x 65.
B = Q diag(linspace(1, 20, n)) W^T with Q (m x n) and W (n x n) from the QR
of Gaussian matrices, so cond(B) = 20; D is a random power of two per column,
down to 2^-40 (fp64) or 2^-20 (fp32).  By Demmel-Veselic, one-sided Jacobi
gets every singular value of such a matrix to a relative error ~ eps cond(B),
whatever D is; LAPACK in float64 does not.

The expected values come from the numpy model of the kernel's method
(tests/jacobi_model.py) run in np.longdouble on exactly the stored (rounded)
matrix; this script refuses to write where longdouble is no wider than
double.  Keys: A_<sfx>_<i>, S_<sfx>_<i> (float64), i = 0 .. 2.

    python tests/golden/make_batched_mid_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from jacobi_model import jacobi_svd  # noqa: E402

SHAPES = [(128, 128), (100, 72), (128, 65)]
KMAX = {"f64": 40, "f32": 20}
DTYPE = {"f64": np.float64, "f32": np.float32}


def graded(rng, m, n, kmax, dtype):
    Q = np.linalg.qr(rng.standard_normal((m, n)))[0]
    W = np.linalg.qr(rng.standard_normal((n, n)))[0]
    B = (Q * np.linspace(1, 20, n)) @ W.T
    k = rng.integers(0, kmax + 1, n)
    return np.ascontiguousarray((B * np.ldexp(1.0, -k)).astype(dtype))


def main():
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than double here: not writing"
    rng = np.random.default_rng(20240902)
    out = {}
    for sfx in ("f64", "f32"):
        for i, (m, n) in enumerate(SHAPES):
            A = graded(rng, m, n, KMAX[sfx], DTYPE[sfx])
            _, S, _, info, sweeps = jacobi_svd(A.astype(np.longdouble), dtype=np.longdouble)
            assert info == 0, f"the model did not converge ({sweeps} sweeps)"
            out[f"A_{sfx}_{i}"] = A
            out[f"S_{sfx}_{i}"] = S.astype(np.float64)
    path = os.path.join(HERE, "batched_graded_mid.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
