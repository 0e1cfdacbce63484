"""Generator of tests/golden/batched_graded_tall.npz: tall graded matrices
whose small singular values only a relatively accurate method gets right --
the QR front end of the batched tall SVD must not lose what the Jacobi kernel
behind it keeps.

Four 300 x 16 matrices A = B D per dtype, built like make_batched_golden.py: B
has unit columns with entries +-uniform(1, 2) before normalisation; D =
diag(2^-k) with k spread over 0..40 (fp64) or 0..20 (fp32); the columns are
then permuted.  300 rows are two row blocks of the 16-column class.

The expected values come from the numpy model of the Jacobi method
(tests/jacobi_model.py) run in np.longdouble on exactly the stored (rounded)
matrix -- on the whole 300 x 16 matrix, with no QR in front; this script
refuses to write where longdouble is no wider than double.

    python tests/golden/make_batched_tall_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from jacobi_model import jacobi_svd  # noqa: E402

COUNT, M, N = 4, 300, 16
KMAX = {"f64": 40, "f32": 20}
DTYPE = {"f64": np.float64, "f32": np.float32}


def graded(rng, kmax, dtype):
    B = rng.uniform(1, 2, (M, N)) * rng.choice([-1.0, 1.0], (M, N))
    B /= np.linalg.norm(B, axis=0)
    k = np.round(np.linspace(0, kmax, N)).astype(int)
    A = B * np.ldexp(1.0, -k)
    return np.ascontiguousarray(A[:, rng.permutation(N)].astype(dtype))


def main():
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than double here: not writing"
    rng = np.random.default_rng(20240612)
    out = {}
    for sfx in ("f64", "f32"):
        As, Ss = [], []
        for _ in range(COUNT):
            A = graded(rng, KMAX[sfx], DTYPE[sfx])
            _, S, _, info, sweeps = jacobi_svd(A.astype(np.longdouble), dtype=np.longdouble)
            assert info == 0, f"the model did not converge ({sweeps} sweeps)"
            As.append(A)
            Ss.append(S.astype(np.float64))
        out[f"A_{sfx}"] = np.stack(As)
        out[f"S_{sfx}"] = np.stack(Ss)
    path = os.path.join(HERE, "batched_graded_tall.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
