"""What every round entry point launches, pinned by a table (no GPU, no libdlamd.so):
tests/launch_sweep.cpp links only csrc/launch.cpp and csrc/plan.cpp, is built here with the host
compiler under the address and undefined-behaviour sanitizers, and runs as an ordinary process
over tests/golden/mix_launches.txt at 256 compute units: every launch, follow-up and refusal of the
table from the pure functions, plus what must hold of any launch list (partial rows disjoint and
inside the workspace, grid <= tiles, every column covered once, hub heads inside LDS).

A line reads
    name entry n_rows nnz uniform_row_nnz doubly_stochastic shared_row_weights min_row_nnz
    n_params tile_cols n_halo n_local_src deviation lagged ldx ldy ldg ldh misalignment
    halo_blocks n_hub_rows ws_misalignment ws_bytes rounds flags knob -> status result
with entry one of round (dl_mix_round), rounds (dl_mix_rounds), trace (dl_mix_rounds_trace), dev
(dl_deviation), devtiled (dl_deviation_tiled) and sgdround (dl_sgd_round); misalignment the bytes
x:y:g:halo[:buf] are off their 16-byte aligned addresses; halo_blocks 0 or n:rows:rows:...; ws_bytes -1 for a null workspace;
flags `-` or a comma list (launch_table.h: g, mean, nodevsq, pro, nullx, y=x, ...); knob `-` or
NAME=value.  The result is the error text, or the launches and then `; follow-up`:
    tile chunks sgd dev mix fast grid lds {TileArgs}
    sgdtile chunks dev fast grid lds {TileArgs} {buf ldb bts brs lr mu damp wd first nesterov}
    reg chunks head tail_fmt sgd dev grid lds {TileArgs}
    gather sgd columns {TileArgs}
    multi chunks rounds sgd dev grid lds {TileArgs}
    trace chunks planes rounds grid lds {TileArgs}
    irr head general_mean narrow rounds grid lds {TileArgs}
    ; none | zero | reduce partial parts rows max_zeroed | partial_rows n | two_pass | trace_reduce
{TileArgs} holds every scalar field in declaration order, a pointer as the byte offset from its
operand's address or `-`, the halo block tables up to n_hblk.

The right sides were recorded from the commit before launch shaping moved out of capi.hip: that
commit's capi.hip and plan.cpp linked against recording stubs of the dl::launch_* functions, run
on the CPU over these left sides.  The sgdround lines (flags mu=, ldb=, damp=, wd=, nest, first,
nullbuf, buf=x|y|g for the momentum buffer and the optimizer) were recorded the same way from the
commit before dl_sgd_round's shaping moved: that commit's capi.hip, plan.cpp and launch.cpp against
recording stubs of launch_mix_sgd_tile, launch_dev_reduce and hipMemsetAsync."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "distributed-learning_amd", "csrc")


def test_sanitized_launch_sweep(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++", path="/opt/rocm/llvm/bin")
    if not cxx:
        pytest.skip("no host C++ compiler (g++ or the ROCm clang++)")
    exe = str(tmp_path / "launch_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "launch_sweep.cpp"), os.path.join(CSRC, "launch.cpp"),
                    os.path.join(CSRC, "plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe, os.path.join(HERE, "golden", "mix_launches.txt")],
                         capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr[:4000]
    assert run.stdout.split()[1:] == ["calls,", "0", "failures"]
