"""The mix planner pinned by a table (no GPU): tests/golden/mix_plans.txt holds one planner query
per line -- entry point, sizes and flags, one knob -- and what the library answered: the status
and every dl_mix_plan field, the traced pass's round cap, or the dl_last_error() text.  The test
replays every line through the ctypes ABI and compares all of it exactly.

A line reads
    name entry n_rows nnz uniform_row_nnz doubly_stochastic shared_row_weights min_row_nnz
    n_params tile_cols n_halo n_local_src deviation lagged knob -> status result
with entry one of query (dl_mix_plan_query), csr (dl_mix_plan_csr, tile_cols -1), rounds
(dl_mix_rounds_plan) and trace (dl_mix_trace_plan); knob `-` or NAME=value; result the plan's
path tile_cols grid lds_bytes n_tiles regular head tail_fmt, or max_rounds, or the error text.
The planner never dereferences an operand, so the pointers are fake addresses.

`python tests/test_plan_table_cpu.py --write` regenerates the table from the library that
DLAMD_LIB names (the build of the commit whose plans are to be kept)."""
import ctypes
import itertools
import os
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mix_plans.txt")
PLAN_FIELDS = ("path", "tile_cols", "grid", "lds_bytes", "n_tiles", "regular", "head", "tail_fmt")
N_CUS = 256   # the table's compute units: device_cus() of an MI355X, and without a device


def device_cus(lib):
    return (lib.dl_mix_trace_workspace_bytes(64, 1) - 256) // 256


def answer(lib, case):
    """The library's answer to one query, as the text after `->`."""
    from distributed_learning_amd import _lib
    (_, entry, n_rows, nnz, uniform, ds, shared, min_nnz, n_params, tile_cols, n_halo, n_local,
     dev, lag, knob) = case
    W = _lib.DlCsr(64, 64, 64, n_rows, nnz, uniform, ds, shared, min_nnz)
    plan, cap = _lib.DlMixPlan(), ctypes.c_int32(0)
    a = _lib.DlMixArgs()
    a.x, a.y, a.halo = 1 << 20, 1 << 40, (1 << 44 if n_halo else None)
    a.ldx = a.ldy = 0 if tile_cols > 0 else n_params
    a.ldh = n_params if n_halo and tile_cols <= 0 else 0
    a.n_params, a.W, a.tile_cols, a.n_halo, a.n_local_src = n_params, W, tile_cols, n_halo, n_local
    if dev:
        a.dev_sq, a.dev_max = 1 << 45, (1 << 45) + (1 << 24)
    if lag:
        a.mean_prev, a.colsum_out = 1 << 46, 1 << 47
    if knob != "-":
        os.environ.__setitem__(*knob.split("="))
    try:
        if entry == "csr":
            rc = lib.dl_mix_plan_csr(ctypes.byref(W), n_halo, n_params, dev, -1, ctypes.byref(plan))
        elif entry == "trace":
            rc = lib.dl_mix_trace_plan(ctypes.byref(a), ctypes.byref(cap))
        else:
            fn = lib.dl_mix_plan_query if entry == "query" else lib.dl_mix_rounds_plan
            rc = fn(ctypes.byref(a), ctypes.byref(plan))
    finally:
        if knob != "-":
            del os.environ[knob.split("=")[0]]
    if rc:
        return f"{rc} {lib.dl_last_error().decode()}"
    if entry == "trace":
        return f"0 {cap.value}"
    return "0 " + " ".join(str(getattr(plan, f)) for f in PLAN_FIELDS)


def parse(line):
    left, want = line.rstrip("\n").split(" -> ")
    f = left.split()
    return (f[0], f[1], *map(int, f[2:14]), f[14]), want


def test_every_plan_of_the_table():
    from distributed_learning_amd import _lib
    lib = _lib.load()
    if device_cus(lib) != N_CUS:
        pytest.skip(f"the table assumes {N_CUS} compute units, this device has {device_cus(lib)}")
    with open(FIXTURE) as f:
        lines = f.readlines()
    assert len(lines) > 1500
    bad = [f"{line.rstrip()}   got: {got}" for line in lines
           for case, want in [parse(line)] for got in [answer(lib, case)] if got != want]
    assert not bad, f"{len(bad)} of {len(lines)} plans differ:\n" + "\n".join(bad[:20])


# ---- the generator -----------------------------------------------------------------------

ROWS = (2, 8, 64, 255, 256, 276, 608, 1024, 1500, 2048, 2176, 3000, 4096, 5000, 70000)
PARAMS = (4, 20, 132, 1024, 4100, 164608, 1 << 18, 1 << 20)
LAYOUTS = (0, 4, 16, 64, 128)
KNOBS = ("DLAMD_GRID_MULT=1", "DLAMD_GRID_MULT=3", "DLAMD_WG_PER_CU=1", "DLAMD_BALANCE_GRID=0",
         "DLAMD_FORCE_REG=1", "DLAMD_FORCE_GATHER=1", "DLAMD_MAX_TILE_CHUNKS=4",
         "DLAMD_TILE_GROUP=1", "DLAMD_TRACE_PLANES=1")


def graph_kinds(n):
    """(nnz, uniform_row_nnz, doubly_stochastic, shared_row_weights, min_row_nnz) of n agents."""
    def irregular(nnz, ds, min_nnz):
        nnz = min(n * n, nnz)
        return nnz, 0, ds, 0, min(min_nnz, nnz // n)
    return (
        (5 * n, 5, 1, 1, 5),              # degree-4 regular, shared weights
        (5 * n, 5, 1, 0, 5),              # ... per-entry weights
        irregular(5 * n - 6, 1, 3),       # Barabasi-Albert m = 2 like
        irregular(3 * n - 2, 0, 1),       # a tree, W row-stochastic only
        irregular(12 * n, 1, 3),          # a tail too dense for path 5
    )


def named_cases():
    from distributed_learning_amd import graph
    rr4 = lambda n, shared=1: (n, 5 * n, 5, 1, shared, 5)
    yield ("c2", "csr", *rr4(1024), 1 << 20, -1, 0, 0, 0, 0)
    yield ("c2", "csr", *rr4(1024), 1 << 20, -1, 0, 0, 1, 0)
    for tc in LAYOUTS:
        yield ("c2", "query", *rr4(1024), 1 << 20, tc, 0, 0, 0, 0)
        yield ("c3", "query", *rr4(256), 164608, tc, 0, 0, 1, 0)
    for shared in (1, 0):
        for dev in (0, 1):
            yield ("c4", "csr", *rr4(4096, shared), 1 << 18, -1, 0, 0, dev, 0)
            yield ("c4", "query", *rr4(4096, shared), 1 << 18, 4, 0, 0, dev, 0)
    for m, seed in ((1, 2), (2, 1)):
        g = graph.barabasi_albert_metropolis(4096, m, seed)
        W = (4096, g.nnz, 0, 1, 0, g.min_row_nnz)
        for entry, tc in (("csr", -1), ("query", 0), ("query", 4), ("trace", 0)):
            yield (f"c4-ba{m}", entry, *W, 1 << 18, tc, 0, 0, 0 if entry == "trace" else 1, 0)
    # the c4 ranks of 8 / 4 / 2: local + halo rows at their tile width
    for local, halo, tc in ((512, 96, 16), (1024, 128, 16), (2048, 128, 4)):
        for lag in (0, 1):
            yield ("c4-rank", "query", *rr4(local), 1 << 18, tc, halo, 0, lag, lag)
            yield ("c4-rank", "csr", *rr4(local), 1 << 18, -1, halo, 0, lag, 0)
    for lag in (0, 1):   # the split scheme's boundary launch
        yield ("c4-split", "query", *rr4(84), 1 << 18, 16, 96, 180, lag, lag)
    # 16 or 32 kernel chunks at exactly 3 row passes, no lagged deviation (and with it)
    for local, halo, tc in ((64, 96, 64), (64, 128, 64), (8, 128, 64), (64, 16, 128),
                            (64, 16, 16), (64, 16, 4)):
        for lag in (0, 1):
            yield ("corner" if not lag else "corner-lag", "query", *rr4(local), 1 << 18, tc,
                   halo, 0, lag, lag)


def swept_cases():
    def thin(cases, stride):
        return itertools.islice(cases, 0, None, stride)

    def local(entry, layouts, devs):
        for n, p in itertools.product(ROWS, PARAMS):
            for kind, tc, dev in itertools.product(graph_kinds(n), layouts, devs):
                yield ("-", entry, n, *kind, p, tc, 0, 0, dev, 0)

    def chosen_width():
        for n, p, halo, dev in itertools.product(ROWS, PARAMS, (0, 16, 96, 128), (0, 1)):
            for kind in graph_kinds(n):
                yield ("-", "csr", n, *kind, p, -1, halo, 0, dev, 0)

    def halo_rounds():   # whole tiles only (n_params % tile_cols == 0)
        for n, p, halo in itertools.product((2, 8, 64, 84, 180, 255, 256, 512, 1024, 1500, 2048,
                                             4096), (1024, 164608, 1 << 18, 1 << 20), (16, 96, 128)):
            for kind, tc, lag, part in itertools.product(graph_kinds(n)[:3], LAYOUTS, (0, 1),
                                                         (0, 1)):
                rows = (n + 1) // 2 if part else n    # outputs: a row set of the local window
                kind = (kind[0] // n * rows,) + kind[1:]
                yield ("-", "query", rows, *kind, p, tc, halo, n if part else 0, lag, lag)

    yield from thin(local("query", LAYOUTS, (0, 1)), 9)
    yield from thin(chosen_width(), 13)
    yield from thin(halo_rounds(), 23)
    yield from thin(local("rounds", LAYOUTS, (0, 1)), 29)
    yield from thin(local("trace", LAYOUTS, (0,)), 17)


def write():
    from distributed_learning_amd import _lib
    lib = _lib.load()
    assert device_cus(lib) == N_CUS
    named, swept = list(named_cases()), list(swept_cases())
    cases = [c + ("-",) for c in named + swept]
    for i, knob in enumerate(KNOBS):   # every knob on the named rows and a slice of the sweep
        cases += [c + (knob,) for c in named + swept[i::40]
                  if (c[1] == "trace") == (knob == "DLAMD_TRACE_PLANES=1")]
    planner_errors = ("does not fit this graph", "gather path", "dl_mix_rounds")
    with open(FIXTURE, "w") as f:
        for case in cases:
            got = answer(lib, case)
            assert got[0] == "0" or any(e in got for e in planner_errors), (case, got)
            f.write(" ".join(map(str, case)) + " -> " + got + "\n")
    print(f"{len(cases)} plans -> {FIXTURE} ({os.path.getsize(FIXTURE)} bytes)")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    write()
