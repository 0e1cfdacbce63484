"""Timing of the batched small-matrix SVD (svd_batched) on the GPU, in one run:

  (a) svd_batched, values only and with vectors;
  (b) the route the library offered before it: a loop of
      singular_values_gpu(A_i, b=min(32, n)) over 64 of the same matrices, per
      matrix (square shapes only);
  (c) torch.linalg.svdvals / torch.linalg.svd on the whole batch.

fp64 and fp32 at batch x m x n = 16384x16x16, 4096x32x32, 2048x64x64 and
1024x128x64, uniform(0, 5) entries from a fixed seed.  Every shape is warmed
up first; each figure is the median of five windows of at least 0.3 s between
device events, with the spread (max - min) of the five.  The sweeps come from
the numpy model of the kernel's method (tests/jacobi_model.py) on the first
two matrices of each batch.

    python tools/bench_batched.py [--out profiles/batched_svd.json] [--skip-torch]

--tall times the batched tall SVD (svd_tall_batched) instead, by the same
method, at batch x m x n = 4096x256x16, 1024x1024x32, 256x4096x64 and
1024x512x64 (default output profiles/batched_svd_tall.json): values and
vectors, torch.linalg.svdvals / svd on the same batch (on its first 128
matrices, recorded as torch_batch, when one call on the whole batch takes more
than a second), the share of the device time in the three stages (QR, Jacobi
on R, back-application; from the library's profile classes over ten calls)
and the values path's HBM rate against A read once.

--mid times the batched mid-size SVD (svd_mid_batched, 65 to 128 columns)
instead, by the same method, at batch x m x n = 1024x96x96, 1024x128x96 and
1024x128x128 (default output profiles/batched_svd_mid.json): values and
vectors and their ratio (in fp64 the vectors class keeps V in device memory),
torch.linalg.svdvals / svd on the same batch (or its first 128 matrices, as
above), the loop of singular_values_gpu(A_i, b=32) over 64 matrices at the
square shapes, and the model's sweeps on the first two matrices.

--tall-mid times the batched tall mid-size SVD (gesvd_batched beyond 128 rows
with 65 to 128 columns) instead, by the method of --tall, at batch x m x n =
1024x512x96, 1024x512x128, 256x4096x128 and 1024x256x72 (default output
profiles/batched_svd_tall_mid.json): values and vectors, the stage shares, the
values path's HBM rate, torch as above, and the loop of singular_values_gpu
over 64 of the matrices padded with zero columns to m x m (the only way the
two-stage path takes them; shapes of at most 512 rows).

--lstsq times the batched least squares (lstsq_batched, pinv_batched) instead,
by the same method, at batch x m x n = 1024x512x128, 1024x256x72, 1024x128x64
and 256x4096x128 (default output profiles/batched_lstsq.json): lstsq_batched at
1 and 16 right-hand sides and pinv_batched; the share of the solve launch in
the call (profile kinds gelss_solve over gelss_batched, ten calls);
gesvd_batched with vectors at the same shape (the cost before the solve);
gesvd_batched followed by the equivalent chain of torch.bmm calls with the
same cutoff; torch.linalg.lstsq / pinv on the first 128 matrices.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import svdsolver_amd as S  # noqa: E402
from jacobi_model import jacobi_svd  # noqa: E402

SHAPES = [(16384, 16, 16), (4096, 32, 32), (2048, 64, 64), (1024, 128, 64)]
TALL_SHAPES = [(4096, 256, 16), (1024, 1024, 32), (256, 4096, 64), (1024, 512, 64)]
MID_SHAPES = [(1024, 96, 96), (1024, 128, 96), (1024, 128, 128)]
TALL_MID_SHAPES = [(1024, 512, 96), (1024, 512, 128), (256, 4096, 128), (1024, 256, 72)]
LSTSQ_SHAPES = [(1024, 512, 128), (1024, 256, 72), (1024, 128, 64), (256, 4096, 128)]
LSTSQ_NRHS = (1, 16)
LOOP_MAX_ROWS = 512   # the two-stage loop pads to m x m
WINDOW_S, REPEATS, LOOP_MATRICES = 0.3, 5, 64
TORCH_SUBSET, TORCH_CALL_S, STAGE_CALLS = 128, 1.0, 10


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def measure(fn):
    """Median and spread (ms per call) of REPEATS windows of >= WINDOW_S."""
    fn()   # warm-up
    torch.cuda.synchronize()
    once = max(window_ms(fn, 1), 1e-3)
    reps = max(1, math.ceil(WINDOW_S * 1e3 / once))
    ts = [window_ms(fn, reps) for _ in range(REPEATS)]
    return {"median_ms": float(np.median(ts)), "spread_ms": float(max(ts) - min(ts)), "calls_per_window": reps}


def per_matrix(r, count):
    return {"median_us": r["median_ms"] * 1e3 / count, "spread_us": r["spread_ms"] * 1e3 / count,
            "calls_per_window": r["calls_per_window"]}


def stage_shares(fn, whole_kind="svd_tall_batched"):
    """Share of the device time of STAGE_CALLS calls in the three stages."""
    torch.cuda.synchronize()
    S.profile_enable(True)
    S.profile_reset()
    for _ in range(STAGE_CALLS):
        fn()
    torch.cuda.synchronize()
    ms = {k: S.profile_query(f"svd_tall_{k}")["ms"] for k in ("qr", "jacobi", "apply")}
    whole = S.profile_query(whole_kind)["ms"]
    S.profile_enable(False)
    out = {k: v / whole for k, v in ms.items()}
    out["call_us"] = whole * 1e3 / STAGE_CALLS
    return out


def tall_rows(args, dev, result):
    for dt in (torch.float64, torch.float32):
        for batch, m, n in TALL_SHAPES:
            g = torch.Generator(device=dev).manual_seed(1234)
            A = torch.rand((batch, m, n), dtype=dt, device=dev, generator=g) * 5
            row = {"dtype": str(dt).replace("torch.", ""), "batch": batch, "m": m, "n": n}
            info = S.svd_tall_batched(A, check=False)[3]
            row["info_nonzero"] = int((info != 0).sum())
            vals = measure(lambda: S.svdvals_tall_batched(A, check=False, sync=False))
            row["svd_tall_batched_values"] = per_matrix(vals, batch)
            row["svd_tall_batched_vectors"] = per_matrix(
                measure(lambda: S.svd_tall_batched(A, check=False, sync=False)), batch)
            row["values_hbm_tb_per_s"] = batch * m * n * A.element_size() / (vals["median_ms"] * 1e-3) / 1e12
            row["stage_share_values"] = stage_shares(lambda: S.svdvals_tall_batched(A, check=False, sync=False))
            row["stage_share_vectors"] = stage_shares(lambda: S.svd_tall_batched(A, check=False, sync=False))
            if not args.skip_torch:
                torch.linalg.svdvals(A[:2])   # library start-up is not the batch's time
                torch.cuda.synchronize()
                At = A if window_ms(lambda: torch.linalg.svdvals(A), 1) <= TORCH_CALL_S * 1e3 else A[:TORCH_SUBSET]
                row["torch_batch"] = At.shape[0]
                row["torch_svdvals"] = per_matrix(measure(lambda: torch.linalg.svdvals(At)), At.shape[0])
                row["torch_svd"] = per_matrix(measure(lambda: torch.linalg.svd(At, full_matrices=False)), At.shape[0])
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "w") as f:   # rewritten after every shape: a cut-short run keeps its rows
                json.dump(result, f, indent=1)
                f.write("\n")


def tall_mid_rows(args, dev, result):
    for dt in (torch.float64, torch.float32):
        for batch, m, n in TALL_MID_SHAPES:
            g = torch.Generator(device=dev).manual_seed(1234)
            A = torch.rand((batch, m, n), dtype=dt, device=dev, generator=g) * 5
            row = {"dtype": str(dt).replace("torch.", ""), "batch": batch, "m": m, "n": n}
            info = S.gesvd_batched(A, check=False)[3]
            row["info_nonzero"] = int((info != 0).sum())
            vals = measure(lambda: S.gesvdvals_batched(A, check=False, sync=False))
            row["gesvd_batched_values"] = per_matrix(vals, batch)
            row["gesvd_batched_vectors"] = per_matrix(
                measure(lambda: S.gesvd_batched(A, check=False, sync=False)), batch)
            row["values_hbm_tb_per_s"] = batch * m * n * A.element_size() / (vals["median_ms"] * 1e-3) / 1e12
            row["stage_share_values"] = stage_shares(lambda: S.gesvdvals_batched(A, check=False, sync=False),
                                                     "gesvd_batched")
            row["stage_share_vectors"] = stage_shares(lambda: S.gesvd_batched(A, check=False, sync=False),
                                                      "gesvd_batched")
            if m <= LOOP_MAX_ROWS:
                P = torch.zeros((LOOP_MATRICES, m, m), dtype=dt, device=dev)
                P[:, :, :n] = A[:LOOP_MATRICES]

                def loop():
                    for i in range(LOOP_MATRICES):
                        S.singular_values_gpu(P[i], b=32)
                row["loop_singular_values_gpu_padded"] = per_matrix(measure(loop), LOOP_MATRICES)
            if not args.skip_torch:
                torch.linalg.svdvals(A[:2])   # library start-up is not the batch's time
                torch.cuda.synchronize()
                At = A if window_ms(lambda: torch.linalg.svdvals(A), 1) <= TORCH_CALL_S * 1e3 else A[:TORCH_SUBSET]
                row["torch_batch"] = At.shape[0]
                row["torch_svdvals"] = per_matrix(measure(lambda: torch.linalg.svdvals(At)), At.shape[0])
                row["torch_svd"] = per_matrix(measure(lambda: torch.linalg.svd(At, full_matrices=False)), At.shape[0])
                row["torch_over_values"] = row["torch_svdvals"]["median_us"] / row["gesvd_batched_values"]["median_us"]
                row["torch_over_vectors"] = row["torch_svd"]["median_us"] / row["gesvd_batched_vectors"]["median_us"]
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "w") as f:   # rewritten after every shape: a cut-short run keeps its rows
                json.dump(result, f, indent=1)
                f.write("\n")


def solve_share(fn):
    """Share of the solve launch in the device time of STAGE_CALLS calls."""
    torch.cuda.synchronize()
    S.profile_enable(True)
    S.profile_reset()
    for _ in range(STAGE_CALLS):
        fn()
    torch.cuda.synchronize()
    solve, whole = S.profile_query("gelss_solve")["ms"], S.profile_query("gelss_batched")["ms"]
    S.profile_enable(False)
    return {"solve_share": solve / whole, "solve_us": solve * 1e3 / STAGE_CALLS, "call_us": whole * 1e3 / STAGE_CALLS}


def bmm_chain(A, B, rcond):
    """What a user of gesvd_batched writes: the cutoff by hand and a chain of
    torch.bmm calls.  B None: the pseudo-inverse."""
    U, Sv, Vh = S.gesvd_batched(A, check=False, sync=False)[:3]
    keep = Sv > rcond * Sv[:, :1]
    inv = torch.where(keep, 1 / Sv, torch.zeros_like(Sv))
    Ut = U.transpose(1, 2)
    C = Ut if B is None else torch.bmm(Ut, B)
    return torch.bmm(Vh.transpose(1, 2), inv.unsqueeze(2) * C)


def torch_row(fn, count):
    try:
        return per_matrix(measure(fn), count)
    except RuntimeError as e:   # a torch build without the batched solver behind this call
        return {"error": str(e).splitlines()[0][:200]}


def lstsq_rows(args, dev, result):
    for dt in (torch.float64, torch.float32):
        for batch, m, n in LSTSQ_SHAPES:
            g = torch.Generator(device=dev).manual_seed(1234)
            A = torch.rand((batch, m, n), dtype=dt, device=dev, generator=g) * 5
            row = {"dtype": str(dt).replace("torch.", ""), "batch": batch, "m": m, "n": n}
            rcond = max(m, n) * torch.finfo(dt).eps
            info = S.gesvd_batched(A, check=False)[3]
            row["info_nonzero"] = int((info != 0).sum())
            row["gesvd_batched_vectors"] = per_matrix(
                measure(lambda: S.gesvd_batched(A, check=False, sync=False)), batch)
            At = A[:TORCH_SUBSET]
            for k in LSTSQ_NRHS:
                B = torch.rand((batch, m, k), dtype=dt, device=dev, generator=g) * 2 - 1
                X, rank = S.lstsq_batched(A, B, check=False)[:2]
                Xc = bmm_chain(A, B, rcond)
                r = {"rank_min": int(rank.min()),
                     "max_diff_to_chain": float((X - Xc).abs().max() / Xc.abs().max())}
                r["lstsq_batched"] = per_matrix(measure(lambda: S.lstsq_batched(A, B, check=False, sync=False)), batch)
                r.update(solve_share(lambda: S.lstsq_batched(A, B, check=False, sync=False)))
                r["gesvd_plus_bmm_chain"] = per_matrix(measure(lambda: bmm_chain(A, B, rcond)), batch)
                r["chain_over_lstsq"] = r["gesvd_plus_bmm_chain"]["median_us"] / r["lstsq_batched"]["median_us"]
                r["lstsq_over_gesvd"] = r["lstsq_batched"]["median_us"] / row["gesvd_batched_vectors"]["median_us"]
                if not args.skip_torch:
                    Bt = B[:TORCH_SUBSET]
                    r["torch_batch"] = At.shape[0]
                    r["torch_lstsq"] = torch_row(lambda: torch.linalg.lstsq(At, Bt), At.shape[0])
                row[f"nrhs_{k}"] = r
            r = {"pinv_batched": per_matrix(measure(lambda: S.pinv_batched(A, check=False, sync=False)), batch)}
            r.update(solve_share(lambda: S.pinv_batched(A, check=False, sync=False)))
            r["gesvd_plus_bmm_chain"] = per_matrix(measure(lambda: bmm_chain(A, None, rcond)), batch)
            r["chain_over_pinv"] = r["gesvd_plus_bmm_chain"]["median_us"] / r["pinv_batched"]["median_us"]
            if not args.skip_torch:
                r["torch_batch"] = At.shape[0]
                r["torch_pinv"] = torch_row(lambda: torch.linalg.pinv(At), At.shape[0])
            row["pinv"] = r
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "w") as f:   # rewritten after every shape: a cut-short run keeps its rows
                json.dump(result, f, indent=1)
                f.write("\n")


def mid_rows(args, dev, result):
    for dt in (torch.float64, torch.float32):
        for batch, m, n in MID_SHAPES:
            g = torch.Generator(device=dev).manual_seed(1234)
            A = torch.rand((batch, m, n), dtype=dt, device=dev, generator=g) * 5
            row = {"dtype": str(dt).replace("torch.", ""), "batch": batch, "m": m, "n": n}
            npdt = np.float64 if dt == torch.float64 else np.float32
            row["model_sweeps"] = [int(jacobi_svd(A[i].cpu().numpy(), dtype=npdt)[4]) for i in range(2)]
            info = S.svd_mid_batched(A, check=False)[3]
            row["info_nonzero"] = int((info != 0).sum())
            vals = measure(lambda: S.svdvals_mid_batched(A, check=False, sync=False))
            vecs = measure(lambda: S.svd_mid_batched(A, check=False, sync=False))
            row["svd_mid_batched_values"] = per_matrix(vals, batch)
            row["svd_mid_batched_vectors"] = per_matrix(vecs, batch)
            row["vectors_over_values"] = vecs["median_ms"] / vals["median_ms"]
            if m == n:
                def loop():
                    for i in range(LOOP_MATRICES):
                        S.singular_values_gpu(A[i], b=32)
                row["loop_singular_values_gpu"] = per_matrix(measure(loop), LOOP_MATRICES)
            if not args.skip_torch:
                torch.linalg.svdvals(A[:2])   # library start-up is not the batch's time
                torch.cuda.synchronize()
                At = A if window_ms(lambda: torch.linalg.svdvals(A), 1) <= TORCH_CALL_S * 1e3 else A[:TORCH_SUBSET]
                row["torch_batch"] = At.shape[0]
                row["torch_svdvals"] = per_matrix(measure(lambda: torch.linalg.svdvals(At)), At.shape[0])
                row["torch_svd"] = per_matrix(measure(lambda: torch.linalg.svd(At, full_matrices=False)), At.shape[0])
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "w") as f:   # rewritten after every shape: a cut-short run keeps its rows
                json.dump(result, f, indent=1)
                f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-torch", action="store_true", help="leave out measurement (c)")
    ap.add_argument("--tall", action="store_true", help="the tall shapes through svd_tall_batched")
    ap.add_argument("--mid", action="store_true", help="the 65..128-column shapes through svd_mid_batched")
    ap.add_argument("--tall-mid", action="store_true",
                    help="more than 128 rows with 65..128 columns through gesvd_batched")
    ap.add_argument("--lstsq", action="store_true", help="lstsq_batched and pinv_batched")
    args = ap.parse_args()
    if args.tall + args.mid + args.tall_mid + args.lstsq > 1:
        ap.error("--tall, --mid, --tall-mid and --lstsq are separate runs")
    if args.out is None:
        name = ("batched_svd_tall.json" if args.tall else "batched_svd_mid.json" if args.mid else
                "batched_svd_tall_mid.json" if args.tall_mid else "batched_lstsq.json" if args.lstsq else
                "batched_svd.json")
        args.out = os.path.join(REPO, "profiles", name)
    args.out = os.path.abspath(args.out)
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(dev)
    result = {"device": props.name, "cus": props.multi_processor_count, "window_s": WINDOW_S, "repeats": REPEATS,
              "unit": "microseconds per matrix", "rows": []}
    if args.tall:
        tall_rows(args, dev, result)
        return
    if args.mid:
        mid_rows(args, dev, result)
        return
    if args.tall_mid:
        tall_mid_rows(args, dev, result)
        return
    if args.lstsq:
        lstsq_rows(args, dev, result)
        return
    for dt in (torch.float64, torch.float32):
        for batch, m, n in SHAPES:
            g = torch.Generator(device=dev).manual_seed(1234)
            A = torch.rand((batch, m, n), dtype=dt, device=dev, generator=g) * 5
            row = {"dtype": str(dt).replace("torch.", ""), "batch": batch, "m": m, "n": n}
            npdt = np.float64 if dt == torch.float64 else np.float32
            row["model_sweeps"] = [int(jacobi_svd(A[i].cpu().numpy(), dtype=npdt)[4]) for i in range(2)]
            info = S.svd_batched(A, check=False)[3]
            row["info_nonzero"] = int((info != 0).sum())
            row["svd_batched_values"] = per_matrix(measure(lambda: S.svdvals_batched(A, check=False, sync=False)), batch)
            row["svd_batched_vectors"] = per_matrix(measure(lambda: S.svd_batched(A, check=False, sync=False)), batch)
            if m == n:
                def loop():
                    for i in range(LOOP_MATRICES):
                        S.singular_values_gpu(A[i], b=min(32, n))
                row["loop_singular_values_gpu"] = per_matrix(measure(loop), LOOP_MATRICES)
            if not args.skip_torch:
                row["torch_svdvals"] = per_matrix(measure(lambda: torch.linalg.svdvals(A)), batch)
                row["torch_svd"] = per_matrix(measure(lambda: torch.linalg.svd(A, full_matrices=False)), batch)
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "w") as f:   # rewritten after every shape: a cut-short run keeps its rows
                json.dump(result, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
