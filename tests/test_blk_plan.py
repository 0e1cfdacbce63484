"""CPU test of the blocked stage 1's launch sizing (svdsolver_amd/csrc/
brd_blk_plan.h: the read passes' split, the prep kernels' grid, the block
update's grid and tile order): tests/cpp/test_blk_plan.cpp is compiled with
g++ (no HIP) and run; it sweeps sizes, targets and switches and checks the
conditions the kernels rely on -- every (tile, stage) of a read pass dealt
exactly once and at most ksmax partial slots per tile, the block update's
tile order a bijection -- as tests/test_stage2_schedule.py does for stage 2."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blk_plan(tmp_path):
    exe = tmp_path / "test_blk_plan"
    src = os.path.join(REPO, "tests", "cpp", "test_blk_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "svdsolver_amd", "csrc"), src, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
