"""The instantiation families of mix_sgd_tile_kernel and mix_cheb_tile_kernel that the GPU tests
launch, from the tests' own parameter lists (no GPU: families.cpp shapes each round in host-only
code).  Run from the repository root: python profiles/r22/tile_core/families.py [extra ...]
where an extra case is kind:n:P:deg:weights:layout:dev (layout rows, pad, pad3 or tiled)."""
import collections
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import special_values as sv  # noqa: E402
import test_cheb_round_gpu as tc  # noqa: E402
import test_sgd_round_gpu as ts  # noqa: E402
from test_mix_gpu import graph_csr  # noqa: E402


def build():
    exe = os.path.join(tempfile.mkdtemp(), "families")
    csrc = os.path.join(ROOT, "distributed-learning_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "tests"),
                    os.path.join(HERE, "families.cpp"), os.path.join(csrc, "launch.cpp"),
                    os.path.join(csrc, "plan.cpp"), "-o", exe], check=True)
    return exe


def line(name, kind, csr, P, layout, dev):
    """layout: rows (ld = P), pad (ld = P + 4), pad3 (ld = P + 3) or tiled (the planner's tile
    width)."""
    tcols = -1 if layout == "tiled" else 0
    ld = P + {"pad": 4, "pad3": 3}.get(layout, 0)
    return (f"{name} {kind} {csr.n_rows} {csr.nnz} {csr.uniform_row_nnz} "
            f"{int(bool(csr.doubly_stochastic))} {int(bool(csr.shared_row_weights))} "
            f"{csr.min_row_nnz} {P} {tcols} {ld} {int(dev)}")


def cases():
    out = []
    dev_shapes = [(256, 1030, 4, "regular"), (300, 777, 8, "random"), (1500, 64, 6, "random"),
                  (64, 4096, 4, "regular"), (64, 4096, 4, "random"), (1024, 4100, 4, "random")]
    for kind in ("sgd", "cheb"):
        for n, P, deg in ts.SHAPES:
            out.append(line(f"bits_{n}x{P}", kind, ts.problem(n, P, deg)[0], P, "rows", False))
        for n, P, deg, w in dev_shapes:
            out.append(line(f"deviation_{n}x{P}_{w}", kind, ts.problem(n, P, deg, w)[0], P, "rows",
                            True))
        for n, P, deg in [(33, 129, 4), (64, 4096, 4), (300, 777, 8)]:
            out.append(line(f"padding_{n}x{P}", kind, ts.problem(n, P, deg)[0], P, "pad", False))
        for n, P, deg in [(64, 4096, 4), (300, 777, 8)]:
            out.append(line(f"tiled_engine_{n}x{P}", kind, ts.problem(n, P, deg)[0], P, "tiled",
                            True))
        for n, tiles, w, dev in ts.FAMILIES:   # the cases added with tile_core.h
            P = ts.family_params(tiles)
            out.append(line(f"families_{n}_{tiles}tiles_{w}_dev{int(dev)}", kind,
                            ts.problem(n, P, 4, w)[0], P, "pad3", dev))
        # three tiles per workgroup plus 4 columns (grid 512 x 128 columns at 64 agents)
        out.append(line("walk_three_tiles", kind, graph_csr(64, 4, seed=5), 3 * 512 * 128 + 4,
                        "rows", False))
        for name, layout in [("fused_33x129", "rows"), ("fused_circ64x256", "tiled")]:
            graph, n, P, _ = sv.SHAPES[name]
            out.append(line("special_" + name, kind, graph(sv.CLASSES[0]), P, layout, True))
    for n, P in [(64, 256), (33, 129)]:
        out.append(line(f"engine_mix_chebyshev_{n}x{P}", "cheb", graph_csr(n, 4, seed=n), P, "rows",
                        True))
    return out


def main():
    lines = cases()
    for extra in sys.argv[1:]:
        kind, n, P, deg, w, layout, dev = extra.split(":")
        csr = ts.problem(int(n), int(P), int(deg), w)[0]
        lines.append(line(f"new_{n}x{P}_{w}_{layout}", kind, csr, int(P), layout, dev == "1"))
    res = subprocess.run([build()], input="\n".join(lines) + "\n", capture_output=True, text=True,
                         check=True).stdout
    print(res, end="")
    fam = collections.defaultdict(set)
    for ln in res.splitlines():
        w = ln.split()
        if w[2] in ("FAST", "guarded"):
            fam[(w[1], w[2], w[4] if w[2] == "FAST" else "KV=8", w[5], w[6], w[7])].add(w[0])
    print("\nfamilies launched (kernel, path, KV, DEV, mean_from_inputs, reg5): cases")
    for k in sorted(fam):
        print(" ", *k, ":", len(fam[k]))


if __name__ == "__main__":
    main()
