"""bench.py's launcher contract on a host without GPUs (CPU suite): asked for
N > 1 GPUs without an external launcher it must refuse loudly -- never run a
silent one-GPU measurement under an N-GPU label (What's missing
item 4)."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_refuses_more_gpus_than_visible():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HIP_VISIBLE_DEVICES"] = ""
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1"],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode != 0
    assert "requested but only" in out.stderr


def test_bench_rejects_world_size_mismatch():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "4", "--steps", "1"],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode != 0
    assert "WORLD_SIZE=2" in out.stderr


def test_torchrun_command_passes_size_through():
    """`python bench.py --gpus N --n 16384`: the spawned torch.distributed.run
    must hand every bench argument to the script (its own parser would take
    "--n" as an ambiguous abbreviation of --nnodes / --nproc-per-node ...)."""
    import importlib.util
    from torch.distributed.run import get_args_parser
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    cmd = bench.torchrun_cmd(2, ["--gpus", "2", "--n", "4096", "--steps", "3", "--warmup", "1"], 29999)
    ns = get_args_parser().parse_args(cmd[3:])
    assert ns.nproc_per_node == "2" and ns.training_script.endswith("bench.py")
    assert ns.training_script_args == ["--gpus", "2", "--size", "4096", "--steps", "3", "--warmup", "1"]


def _free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


@pytest.mark.gpu
def test_bench_two_ranks_end_to_end():
    """The driver's N > 1 bench path, end to end on one GPU: two ranks under
    torch.distributed.run, stage 1 sharded over them, bands gathered on rank
    j mod 2, stage 2 beside the next matrices, the lanes' communicators --
    through the host-callback communicator (RCCL needs one GPU per rank).
    Rank 0 prints one JSON line with n_gpus = 2 and a positive value."""
    import json
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", f"--master-port={_free_port()}", os.path.join(REPO, "bench.py"),
           "--gpus", "2", "--comm", "host", "--size", "1024", "--steps", "3", "--warmup", "1",
           "--lanes", "2", "--cpu-baseline", "off", "--full"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["config"]["n"] == 1024
    assert d["config"]["matrices_per_timed_region"] == 3


@pytest.mark.gpu
def test_bench_eight_ranks_end_to_end():
    """bench.py --gpus 8 as the driver launches it on an 8-GPU node (configs[4]'s
    P = 8 layout: 8 ranks x the lanes' communicators), rehearsed on one GPU
    through the host-callback communicator at n = 2048 (the blocked path with
    the sharded row-panel CholeskyQR)."""
    import json
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8",
           "--master-addr", "127.0.0.1", f"--master-port={_free_port()}", os.path.join(REPO, "bench.py"),
           "--gpus", "8", "--comm", "host", "--size", "2048", "--steps", "2", "--warmup", "1",
           "--lanes", "2", "--cpu-baseline", "off", "--full"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=400, env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["value"] > 0 and d["config"]["n"] == 2048
    assert d["config"]["matrices_per_timed_region"] == 2


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain one-GPU run: the line holds the headline figure and none of the
    --full measurements, and --dump-outputs writes the last timed step's
    matrix (every step reduces a copy of the same seeded input): its diagonal
    and superdiagonal are the bidiagonal that the same two library calls
    compute here from that input.  The bound is smoke()'s for the fast stage 2
    (1e-8 in the relative 2-norm of |d|, |e|: the stream's launches are sized
    for a shared chip, so the order of its sums may differ)."""
    import json
    import numpy as np
    import torch
    import svdsolver_amd as S
    n, b, steps = 512, 32, 3
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--size", str(n),
                          "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(tmp_path / "o")],
                         capture_output=True, text=True, timeout=240, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["config"]["matrices_per_timed_region"] == steps
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["dtype"] == "f64"
    assert line["value"] == pytest.approx(8.0 / 3.0 * n ** 3 / (line["ms_per_step"] * 1e-3) / 1e9, rel=1e-2)
    for key in ("one_at_a_time", "roofline", "kernel_ms_per_step", "cpu_baseline"):
        assert key not in line
    d, e, full = (np.load(tmp_path / "o" / f"{name}.npy") for name in ("d", "e", "matrix"))
    assert d.dtype == e.dtype == full.dtype == np.float64
    assert d.shape == (n,) and e.shape == (n - 1,) and full.shape == (n, n)
    assert np.array_equal(np.diagonal(full), d) and np.array_equal(np.diagonal(full, 1), e)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1234)
    A = torch.rand((n, n), dtype=torch.float64, device="cuda:0", generator=g) * 5.0
    S.ge2band(A, b)
    d_ref, e_ref = (x.cpu().numpy() for x in S.band2bd(A, b))
    for got, ref in ((d, d_ref), (e, e_ref)):
        err = np.linalg.norm(np.abs(got) - np.abs(ref)) / np.linalg.norm(ref)
        print(f"dumped bidiagonal vs in-process: {err:.2e}")
        assert err < 1e-8
