"""CPU check of the BUILT gfx950 code object (no GPU): the instantiations of mix_dense_kernel are
those the launcher reaches (mix_dense.hip launch_mix_dense: N_pad in {32, 64, 128, 256}, FAST and
guarded) and none uses scratch memory.  The kernel keeps a wave's W fragments for all k in
registers for its whole life (128 at N_pad = 256) beside the prefetched tile; a spill there is a
private-segment round trip per MFMA.  Reads the kernels' metadata notes only (llvm-readelf
--notes), as tests/test_track_resources.py does."""
import re
import subprocess

from test_kernel_isa import LIB, LLVM, code_objects, pytestmark  # noqa: F401

NAME = re.compile(r"_ZN2dl12_GLOBAL__N_116mix_dense_kernelILi(\d+)ELb([01])EEEvNS_9DenseArgsE$")


def test_every_reachable_instantiation_and_none_with_scratch(code_objects):
    notes = {}
    for co in code_objects:
        text = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], capture_output=True,
                              text=True, check=True).stdout
        for entry in re.split(r"\n\s+- (?=\.)", text):   # one YAML map per kernel
            m = re.search(r"\.name:\s+(\S+)", entry)
            if m and NAME.match(m.group(1)):
                notes[m.group(1)] = {k: int(v) for k, v in re.findall(
                    r"\.(private_segment_fixed_size|vgpr_count|vgpr_spill_count|"
                    r"max_flat_workgroup_size):\s+(\d+)", entry)}
    seen = {tuple(int(v) for v in NAME.match(n).groups()) for n in notes}
    assert seen == {(np, fast) for np in (32, 64, 128, 256) for fast in (0, 1)}, sorted(seen)
    for name, f in sorted(notes.items()):
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0, (name, f)
        # 512 threads: two waves a SIMD, 256 registers each (vector and accumulation together)
        assert 0 < f["vgpr_count"] <= 256 and f["max_flat_workgroup_size"] == 512, (name, f)
