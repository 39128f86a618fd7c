"""CPU check of the BUILT gfx950 code object (no GPU): no instantiation of mix_cheb_multi_kernel
uses scratch or more than the 128 VGPRs of a 1024-thread workgroup (from the metadata notes); and
cheb_rounds_sweep.cpp (the launch shaping, host code alone) built and run under ASan / UBSan."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_isa import LIB, LLVM, code_objects, pytestmark  # noqa: F401

NAME = re.compile(r"_ZN2dl12_GLOBAL__N_121mix_cheb_multi_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)"
                  r"ELi(\d+)EEEvNS_8TileArgsENS_13ChebMultiArgsEi$")
FIELDS = r"\.(private_segment_fixed_size|vgpr_count|vgpr_spill_count|max_flat_workgroup_size)"


def test_no_instantiation_uses_scratch_or_more_than_128_vgprs(code_objects):
    notes = {}
    for co in code_objects:
        text = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], capture_output=True,
                              text=True, check=True).stdout
        for entry in re.split(r"\n\s+- (?=\.)", text):
            m = re.search(r"\.name:\s+(\S+)", entry)
            if m and NAME.match(m.group(1)):
                notes[m.group(1)] = {k: int(v) for k, v in re.findall(FIELDS + r":\s+(\d+)", entry)}
    assert len(notes) == 90, sorted(notes)   # (C, KV, OUT, RE, MODE) of mix_cheb_multi.hip's dispatch
    for name, f in sorted(notes.items()):
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0, (name, f)
        assert 0 < f["vgpr_count"] <= 128, (name, f)
        assert f["max_flat_workgroup_size"] == 1024, (name, f)


def test_sanitized_cheb_rounds_sweep(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "distributed-learning_amd", "csrc")
    cxx = shutil.which("g++") or shutil.which("clang++", path="/opt/rocm/llvm/bin")
    if not cxx:
        pytest.skip("no host C++ compiler (g++ or the ROCm clang++)")
    exe = str(tmp_path / "cheb_rounds_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(here, "cheb_rounds_sweep.cpp"), os.path.join(csrc, "launch.cpp"),
                    os.path.join(csrc, "plan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr[:4000]
    words = run.stdout.split()
    assert words[1:] == ["shaped,", "0", "failures"] and int(words[0]) >= 150
