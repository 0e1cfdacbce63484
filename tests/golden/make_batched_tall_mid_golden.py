"""Generator of tests/golden/batched_graded_tall_mid.npz: tall graded matrices
with 65 to 128 columns whose small singular values only a relatively accurate
method gets right -- the 128-column QR front end must not lose what the
mid-size Jacobi kernel behind it keeps.

Two 300 x 72 matrices and one 257 x 128 matrix A = B D per dtype, built like
make_batched_mid_golden.py: B = Q diag(linspace(1, 20, n)) W^T with Q (m x n)
and W (n x n) from the QR of Gaussian matrices, so cond(B) = 20; D is a random
power of two per column, down to 2^-40 (fp64) or 2^-20 (fp32).  300 and 257
rows are three row blocks of 128, the last one ragged (44 rows, 1 row).

The expected values come from the numpy model of the Jacobi method
(tests/jacobi_model.py) run in np.longdouble on exactly the stored (rounded)
matrix -- on the whole matrix, with no QR in front; this script refuses to
write where longdouble is no wider than double.  It also runs the
working-precision model of the whole route (tests/tall_mid_model.py) on every
matrix and refuses to write if that leaves mid_model.graded_limit.
Keys: A_<sfx>_<i>, S_<sfx>_<i> (float64), i = 0 .. 2.

    python tests/golden/make_batched_tall_mid_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from jacobi_model import jacobi_svd  # noqa: E402
from mid_model import graded_limit  # noqa: E402
from tall_mid_model import tall_mid_svd  # noqa: E402

SHAPES = [(300, 72), (300, 72), (257, 128)]
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
    rng = np.random.default_rng(20241020)
    out = {}
    for sfx in ("f64", "f32"):
        worst = 0.0
        for i, (m, n) in enumerate(SHAPES):
            A = graded(rng, m, n, KMAX[sfx], DTYPE[sfx])
            _, S, _, info, sweeps = jacobi_svd(A.astype(np.longdouble), dtype=np.longdouble)
            assert info == 0, f"the model did not converge ({sweeps} sweeps)"
            ref = S.astype(np.float64)
            Sm, im = tall_mid_svd(A, dtype=DTYPE[sfx])[1::2]
            rel = float(np.max(np.abs(Sm.astype(np.float64) - ref) / ref))
            assert im == 0 and rel <= graded_limit(n, DTYPE[sfx]), f"the working-precision model misses: {rel:.2e}"
            worst = max(worst, rel)
            out[f"A_{sfx}_{i}"] = A
            out[f"S_{sfx}_{i}"] = ref
        print(f"{sfx}: the working-precision model's worst relative error {worst:.2e}")
    path = os.path.join(HERE, "batched_graded_tall_mid.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
