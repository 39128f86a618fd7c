"""What dl_adam_round launches, checked against the plain round's launch shaping (no GPU, no
libdlamd.so): tests/adam_sweep.cpp links only csrc/launch.cpp and csrc/plan.cpp, is built here
with the host compiler under the address and undefined-behaviour sanitizers (the flags of
test_track_sweep_cpu.py), and runs as an ordinary process at 256 compute units over

    agents 2, 33, 64, 300, 1024, 1500  x  parameters 7, 129, 777, 4096, 4100
    x  row-major (ld = P and P + 4) and column-tiled  x  with and without deviation
    x  a regular doubly stochastic and an irregular row-stochastic graph
    x  x' apart or x itself  x  the coefficients by value or from the device,

the three option sets (plain, L2, decoupled) in turn.

Every shaped call's launch list must equal shape_round's for the same dl_mix_args in grid, LDS,
chunks, fast and TileArgs, every launch a kLaunchAdamTile whose moment strides are x's and whose
constants are the call's, every column covered once; plan paths 2, 4 and 5 (forced by the knobs,
and where the planner chooses them), every illegal overlap, missing operand, bad stride, bad
parameter and halo / partition / lagged field must be refused with the header's text, by the
round and by its plan query alike."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "distributed-learning_amd", "csrc")


def test_sanitized_adam_sweep(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++", path="/opt/rocm/llvm/bin")
    if not cxx:
        pytest.skip("no host C++ compiler (g++ or the ROCm clang++)")
    exe = str(tmp_path / "adam_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "adam_sweep.cpp"), os.path.join(CSRC, "launch.cpp"),
                    os.path.join(CSRC, "plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr[:4000]
    words = run.stdout.split()
    assert words[1] == "cases," and words[3] == "shaped," and words[4:] == ["0", "failures"]
    assert int(words[0]) >= 1000 and int(words[2]) >= 1000
