"""The .amdhsa_kernel table of a device-only assembly file (make asm RES_SRC=...), and the
comparison of two of them.

  kernel_table.py table FILE.s              name vgpr sgpr scratch lds, one kernel per line
  kernel_table.py diff BEFORE.s AFTER.s     names gained / lost, rows that differ, and how many
                                            kernels have identical instruction text
"""
import re
import sys

KEYS = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def parse(path):
    """{kernel: (resources tuple, instruction text)}"""
    text = open(path).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        body = m.group(2)
        res[m.group(1)] = tuple(int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1)) for k in KEYS)
    code = {}
    for name in res:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), text, re.S | re.M)
        lines = []
        for ln in m.group(1).splitlines():
            ln = ln.split(";")[0].strip()
            # labels carry a per-file function number: .LBB12_3 -> .LBB_3
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            if ln and not ln.startswith("."):
                lines.append(ln)
            elif ln.startswith(".LBB"):
                lines.append(ln)
        code[name] = "\n".join(lines)
    return {k: (res[k], code[k]) for k in res}


def main():
    if sys.argv[1] == "table":
        t = parse(sys.argv[2])
        print("# name vgpr sgpr scratch lds")
        for k in sorted(t):
            print(k, *t[k][0])
        return 0
    a, b = parse(sys.argv[2]), parse(sys.argv[3])
    lost, gained = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    print(f"kernels: {len(a)} before, {len(b)} after; lost {len(lost)}, gained {len(gained)}")
    for k in lost:
        print("  lost  ", k)
    for k in gained:
        print("  gained", k)
    both = sorted(set(a) & set(b))
    differ = [k for k in both if a[k][0] != b[k][0]]
    print(f"resource rows that differ: {len(differ)}   (vgpr sgpr scratch lds)")
    bad = 0
    for k in differ:
        ra, rb = a[k][0], b[k][0]
        flag = ""
        if rb[2] > ra[2]:
            flag += " SCRATCH-UP"
        if ra[0] <= 64 < rb[0]:
            flag += " CROSSES-64"
        bad += bool(flag)
        print(f"  {k}: {ra} -> {rb}{flag}")
    same = sum(a[k][1] == b[k][1] for k in both)
    print(f"identical instruction text: {same} of {len(both)}")
    print(f"kernels with scratch: {sum(v[0][2] > 0 for v in a.values())} before, "
          f"{sum(v[0][2] > 0 for v in b.values())} after")
    return 1 if (bad or lost or gained) else 0


if __name__ == "__main__":
    sys.exit(main())
