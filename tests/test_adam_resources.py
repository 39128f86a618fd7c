"""CPU check of the BUILT gfx950 code object (no GPU): no instantiation of mix_adam_tile_kernel
uses scratch memory, and every one fits the 128 VGPRs of a 1024-thread workgroup.  The kernel
streams four inputs and decides per rows-per-thread which of them ride the cross-tile prefetch
(mix_adam.hip); one stream too many, or one staging step too wide, spills at once, and a spill is
a private-segment round trip per thread and tile.  Reads the kernels' metadata notes only
(llvm-readelf --notes), as test_track_resources.py does."""
import re
import subprocess

from test_kernel_isa import LIB, LLVM, code_objects, pytestmark  # noqa: F401

NAME = re.compile(r"_ZN2dl12_GLOBAL__N_120mix_adam_tile_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])E"
                  r"EEvNS_8TileArgsENS_12AdamTileArgsE$")


def kernel_notes(code_objects):
    """{mangled name: {field: int}} of every mix_adam_tile_kernel in the code objects."""
    out = {}
    for co in code_objects:
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], capture_output=True,
                               text=True, check=True).stdout
        if "mix_adam_tile_kernel" not in notes:
            continue
        # one YAML map per kernel under amdhsa.kernels, each starting with "  - "
        for entry in re.split(r"\n\s+- (?=\.)", notes):
            m = re.search(r"\.name:\s+(\S+)", entry)
            if not m or not NAME.match(m.group(1)):
                continue
            out[m.group(1)] = {k: int(v) for k, v in
                               re.findall(r"\.(private_segment_fixed_size|vgpr_count|"
                                          r"vgpr_spill_count|max_flat_workgroup_size):\s+(\d+)",
                                          entry)}
    return out


def test_no_instantiation_uses_scratch_or_more_than_128_vgprs(code_objects):
    notes = kernel_notes(code_objects)
    seen = {tuple(int(v) for v in NAME.match(n).groups()) for n in notes}
    # FAST: every C x KV in {2, 4, 8}; guarded: every C at 8 rows; each with and without deviation
    want = {(c, kv, dev, 1) for c in (1, 2, 4, 8, 16, 32) for kv in (2, 4, 8) for dev in (0, 1)}
    want |= {(c, 8, dev, 0) for c in (1, 2, 4, 8, 16, 32) for dev in (0, 1)}
    assert seen == want, (sorted(want - seen), sorted(seen - want))
    for name, f in sorted(notes.items()):
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0, (name, f)
        assert 0 < f["vgpr_count"] <= 128, (name, f)
        assert f["max_flat_workgroup_size"] == 1024, (name, f)
