"""The numpy model of the one-sided Jacobi SVD (tests/jacobi_model.py) at 65
to 128 columns against numpy.linalg.svd of the float64 input, in float64 and
float32, under the limits of tests/mid_model.py (jacobi_model.LIMITS times
n / 64) that tests/test_gpu_svd_mid_batched.py applies to the kernel.

This shows that the method alone stays inside them: the model's worst measure
is V orthogonality in fp32 at 128 x 127, 2.6e-4 against a limit of 9.9e-4; it
needs 11 to 12 sweeps at 128 columns."""
import os

import numpy as np
import pytest

from jacobi_model import jacobi_svd, step_pairs
from mid_model import check_svd_mid, graded_limit, rank_deficient_mid

DT = {"f64": np.float64, "f32": np.float32}


def model_inputs():
    cases = [(f"uniform{m}x{n}", np.random.default_rng(1000 * m + n).uniform(0, 5, (m, n)))
             for m, n in ((65, 65), (66, 65), (97, 96), (128, 65), (128, 127), (128, 128))]
    cases.append(("rankdef128x100", rank_deficient_mid(np.random.default_rng(128100))))
    cases.append(("zeros128x128", np.zeros((128, 128))))
    cases.append(("identity128", np.eye(128)))
    return cases


CASES = model_inputs()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("name,A", CASES, ids=[c[0] for c in CASES])
def test_model_against_numpy(name, A, sfx):
    dtype = DT[sfx]
    A64 = A.astype(dtype).astype(np.float64)   # the rounded input is the matrix decomposed
    U, S, V, info, sweeps = jacobi_svd(A64, dtype=dtype)
    assert U.dtype == dtype and S.dtype == dtype and V.dtype == dtype
    assert info == 0, f"sweep cap reached ({sweeps} sweeps)"
    e = check_svd_mid(A64, U, S, V, dtype)
    print(f"{name} {sfx}: {sweeps} sweeps, values {e[0]:.2e} reconstruction {e[1]:.2e} V {e[2]:.2e} U {e[3]:.2e}")


def test_limits_scale_with_the_columns():
    from jacobi_model import LIMITS
    from mid_model import mid_limits
    assert mid_limits(64, np.float64) == LIMITS[np.float64] and mid_limits(16, np.float32) == LIMITS[np.float32]
    assert mid_limits(128, np.float64) == (2e-13, 4e-13, 2e-12)
    assert np.allclose(mid_limits(128, np.float32), (4e-5, 1e-4, 1e-3), rtol=1e-12)
    assert np.allclose(mid_limits(96, np.float64), (1.5e-13, 3e-13, 1.5e-12), rtol=1e-12)


@pytest.mark.parametrize("n", [65, 96, 127, 128])
def test_schedule_meets_every_pair_once(n):
    seen = set()
    for k in range(((n + 1) & ~1) - 1):
        P, Q = step_pairs(n, k)
        cols = np.concatenate([P, Q])
        assert len(set(cols.tolist())) == cols.size, "pairs of a step are disjoint"
        assert np.all(P < Q) and cols.max() < n
        assert P.size == n // 2
        seen |= set(zip(P.tolist(), Q.tolist()))
    assert len(seen) == n * (n - 1) // 2


def test_golden_values_are_the_longdouble_models(golden_dir):
    """The 100 x 72 fp64 matrix of the golden file: its stored values are what
    the model gives in np.longdouble, and the float64 model meets the graded
    limit that the kernel has to meet."""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than double here"
    g = np.load(os.path.join(golden_dir, "batched_graded_mid.npz"))
    assert sorted(g.files) == sorted(f"{k}_{s}_{i}" for k in "AS" for s in DT for i in range(3))
    shapes = [(128, 128), (100, 72), (128, 65)]
    for sfx, dtype in DT.items():
        for i, (m, n) in enumerate(shapes):
            assert g[f"A_{sfx}_{i}"].shape == (m, n) and g[f"A_{sfx}_{i}"].dtype == dtype
            assert g[f"S_{sfx}_{i}"].shape == (n,) and g[f"S_{sfx}_{i}"].dtype == np.float64
    A, ref = g["A_f64_1"], g["S_f64_1"]
    _, S, _, info, _ = jacobi_svd(A.astype(np.longdouble), dtype=np.longdouble)
    assert info == 0
    assert np.array_equal(S.astype(np.float64), ref)
    _, S64, _, info, _ = jacobi_svd(A, dtype=np.float64)
    assert info == 0
    assert np.max(np.abs(S64 - ref) / ref) <= graded_limit(72, np.float64)
