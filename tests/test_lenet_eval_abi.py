"""CPU checks of dl_lenet_eval's C ABI: the struct layout agrees between C and ctypes, the symbols
are additive (ABI still 10), the workspace holds two numbers per 64 rows, the plan query follows
the header's rules, every refusal the header states comes back with its status and its own
message before any device call (dummy pointers, runs without a GPU), and the host-only shaping
(csrc/launch.cpp shape_lenet_eval) walks every block once inside a disjoint workspace -- the
latter from tests/lenet_eval_sweep.cpp, built with the address and undefined-behaviour
sanitizers and run as an ordinary process."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-learning_amd", "csrc")

FIELDS = ["n_agents", "rows", "num_classes", "X", "ldx", "data", "s_data", "labels", "s_labels",
          "loss", "correct", "logits", "ldz", "s_logits", "row_splits"]
PLAN_FIELDS = ["blocks", "row_splits", "grid", "lds_bytes"]


def test_struct_layout_matches_c(tmp_path):
    from distributed_learning_amd import _lib
    offs = "".join(f'printf("%zu ", offsetof(dl_lenet_eval_args, {f}));' for f in FIELDS)
    offs += "".join(f'printf("%zu ", offsetof(dl_lenet_eval_plan, {f}));' for f in PLAN_FIELDS)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dlamd.h"\n'
                    'int main(void){printf("%zu %zu ", sizeof(dl_lenet_eval_args), '
                    'sizeof(dl_lenet_eval_plan));' + offs + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                        check=True).stdout.split()]
    A, Pl = _lib.DlLenetEvalArgs, _lib.DlLenetEvalPlan
    assert [f for f, _ in A._fields_] == FIELDS and [f for f, _ in Pl._fields_] == PLAN_FIELDS
    assert c == [ctypes.sizeof(A), ctypes.sizeof(Pl)] + [getattr(A, f).offset for f in FIELDS] + \
        [getattr(Pl, f).offset for f in PLAN_FIELDS]


def test_symbols_are_additive():
    from distributed_learning_amd import _lib
    lib = _lib.load()
    for name in ("dl_lenet_eval_workspace_bytes", "dl_lenet_eval_plan_query", "dl_lenet_eval"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.dl_abi_version() == 10 == _lib.ABI_VERSION


def test_workspace():
    from distributed_learning_amd import _lib
    lib = _lib.load()
    ws = lib.dl_lenet_eval_workspace_bytes
    base = ws(4, 10000)
    assert base >= 4 * 157 * 8 and base % 16 == 0
    assert ws(400, 10000) > base and ws(4, 100000) > base          # agents, rows
    assert ws(1, 64) == ws(1, 1) and ws(64, 129) >= 64 * 3 * 8      # whole blocks of 64 rows
    assert ws(0, 64) == 0 and ws(4, 0) == 0
    big = ws(65535, 10 ** 6)
    assert big >= 65535 * 15625 * 8 > 2 ** 32                       # size_t, no 32-bit wrap
    # no class argument at all, and far below the training workspace the chunked path sizes
    for n, rows in ((1, 64), (64, 512), (64, 10000), (600, 130)):
        blocks = -(-rows // 64)
        assert ws(n, rows) < blocks * lib.dl_lenet_workspace_bytes(n, 64, 10)
        assert ws(n, rows) < lib.dl_lenet_workspace_bytes(n, 64, 10)
    # on the order of 8 bytes a block: within the two regions' 256-byte rounding
    assert ws(64, 10000) <= 64 * 157 * 8 + 2 * 256


# dummy device addresses, never dereferenced, far apart
X, DATA, LABELS, LOSS, CORRECT, LOGITS, WS = (1 << 40, 1 << 44, 1 << 46, 1 << 48, 1 << 50,
                                              1 << 51, 1 << 52)
N, R, NC = 8, 150, 10
P = 62006
LD = 62016


def valid(**kw):
    from distributed_learning_amd import _lib
    a = _lib.DlLenetEvalArgs(N, R, NC, X, LD, DATA, R * 3072, LABELS, R, LOSS, CORRECT, LOGITS,
                             16, R * 16, 0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def plan(a):
    from distributed_learning_amd import _lib
    lib = _lib.load()
    pl = _lib.DlLenetEvalPlan()
    rc = lib.dl_lenet_eval_plan_query(ctypes.byref(a), ctypes.byref(pl))
    return rc, pl, lib.dl_last_error()


def test_plan_query():
    from distributed_learning_amd import _lib
    for rows in (1, 63, 64, 65, 129, 10000):
        blocks = -(-rows // 64)
        kw = dict(rows=rows, s_data=rows * 3072, s_labels=rows, s_logits=rows * 16)
        rc, pl, msg = plan(valid(**kw))
        assert rc == _lib.DL_OK, msg
        assert pl.blocks == blocks and 1 <= pl.row_splits <= blocks
        assert pl.grid == N * pl.row_splits
        assert 0 < pl.lds_bytes <= 160 * 1024
        auto = pl.row_splits
        for hint, want in ((1, 1), (2, min(2, blocks)), (blocks, blocks), (blocks + 1, blocks),
                           (10 ** 6, blocks)):
            rc, pl, msg = plan(valid(row_splits=hint, **kw))
            assert rc == _lib.DL_OK and (pl.blocks, pl.row_splits, pl.grid) == \
                (blocks, want, N * want), (rows, hint, msg)
        # more agents never get more workgroups each
        rc, pl, _ = plan(valid(n_agents=4096, **kw))
        assert rc == _lib.DL_OK and pl.row_splits <= auto and pl.grid == 4096 * pl.row_splits
    # the query has no workspace and refuses what the call refuses
    rc, _, msg = plan(valid(rows=0))
    assert rc == _lib.DL_ERR_INVALID and b"rows must be >= 1" in msg
    lib = _lib.load()
    assert lib.dl_lenet_eval_plan_query(ctypes.byref(valid()), None) == _lib.DL_ERR_INVALID
    assert b"plan is NULL" in lib.dl_last_error()


def call(a, ws=WS, ws_bytes=None):
    """(status, message) of a call that must be refused before any device call."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    if ws_bytes is None:
        ws_bytes = lib.dl_lenet_eval_workspace_bytes(max(a.n_agents, 1), max(a.rows, 1)) if a \
            else 0
    rc = lib.dl_lenet_eval(ctypes.byref(a) if a is not None else None, ws, ws_bytes, None)
    return rc, lib.dl_last_error()


def test_refusals():
    from distributed_learning_amd import _lib
    INV, UNS, WSP = _lib.DL_ERR_INVALID, _lib.DL_ERR_UNSUPPORTED, _lib.DL_ERR_WORKSPACE
    seen = set()

    def refused(a, status, text, **kw):
        rc, msg = call(a, **kw)
        assert rc == status and text in msg, (rc, msg)
        seen.add(text)

    refused(None, INV, b"args is NULL")
    for f in ("X", "data"):
        refused(valid(**{f: None}), INV, b"null X or data")
    refused(valid(loss=None, correct=None, logits=None), INV, b"no output")
    refused(valid(labels=None), INV, b"loss and correct need labels")
    refused(valid(labels=None, correct=None), INV, b"loss and correct need labels")
    refused(valid(labels=None, loss=None), INV, b"loss and correct need labels")
    for v in (0, -1):
        refused(valid(n_agents=v), INV, b"n_agents must be >= 1")
        refused(valid(rows=v), INV, b"rows must be >= 1")
    refused(valid(n_agents=65536), INV, b"at most 65535 agents")
    for nc in (0, -2):
        refused(valid(num_classes=nc), INV, b"num_classes must be >= 1")
    for nc in (65, 1000):
        refused(valid(num_classes=nc, ldx=1 << 20), UNS, b"at most 64 classes")
    for f, p in (("X", X), ("data", DATA)):
        for off in (4, 8):
            refused(valid(**{f: p + off}), INV, b"X and data must be 16-byte aligned")
    for ld in (P - 2, P + 1, LD + 2, 0, -LD):
        refused(valid(ldx=ld), INV, b"ldx must be a multiple of 4")
    for sd in (R * 3072 - 4, R * 3072 + 2, 4, -R * 3072):
        refused(valid(s_data=sd), INV, b"s_data must be 0 (shared) or a multiple of 4")
    for sl in (R - 1, 1, -R):
        refused(valid(s_labels=sl), INV, b"s_labels must be 0 (shared) or >= rows")
    refused(valid(ldz=NC - 1), INV, b"logits need ldz >= num_classes")
    refused(valid(s_logits=(R - 1) * 16 + NC - 1), INV, b"logits need ldz >= num_classes")
    for rs in (-1, -1000):
        refused(valid(row_splits=rs), INV, b"row_splits must be >= 0")
    refused(valid(n_agents=65535, rows=1 << 30, s_data=0, s_labels=0, logits=None,
                  row_splits=1 << 20), INV, b"grid too large")
    # the workspace: null, misaligned, one byte short
    need = _lib.load().dl_lenet_eval_workspace_bytes(N, R)
    refused(valid(), WSP, b"16-byte aligned workspace", ws=None)
    refused(valid(), WSP, b"16-byte aligned workspace", ws=WS + 4, ws_bytes=need + 4)
    refused(valid(), WSP, b"16-byte aligned workspace", ws_bytes=need - 1)
    assert len(seen) == 17                                  # each refusal has its own message
    # the messages are decided on the host: the other forms pass every check up to the
    # workspace, which is refused here so that nothing is launched
    for kw in (dict(loss=None), dict(correct=None), dict(loss=None, correct=None, labels=None),
               dict(s_data=0, s_labels=0), dict(logits=None), dict(ldx=P + 2),
               dict(num_classes=64, ldz=64, ldx=66596, s_logits=R * 64),
               dict(num_classes=1, ldz=1, s_logits=R), dict(row_splits=7),
               dict(n_agents=65535, rows=1, s_data=3072, s_labels=1, s_logits=16),
               dict(n_agents=2, rows=400000, s_data=0, s_labels=0, logits=None)):   # > 4 GiB
        rc, msg = call(valid(**kw), ws_bytes=0)
        assert rc == WSP, (kw, msg)


def test_overlap_refusals():
    from distributed_learning_amd import _lib
    INV = _lib.DL_ERR_INVALID
    need = _lib.load().dl_lenet_eval_workspace_bytes(N, R)
    x_bytes = ((N - 1) * LD + P) * 4
    d_bytes = N * R * 3072 * 4
    l_bytes = N * R * 4
    z_bytes = ((N - 1) * R * 16 + (R - 1) * 16 + NC) * 4
    cases = [
        (dict(loss=X + 1024), {}, b"loss overlaps X"),
        (dict(loss=X + x_bytes - 4), {}, b"loss overlaps X"),
        (dict(loss=DATA + d_bytes - 4), {}, b"loss overlaps data"),
        (dict(loss=LABELS + l_bytes - 4), {}, b"loss overlaps labels"),
        (dict(correct=X), {}, b"correct overlaps X"),
        (dict(correct=DATA - N * 4 + 4), {}, b"correct overlaps data"),
        (dict(correct=LABELS), {}, b"correct overlaps labels"),
        (dict(logits=X + 64), {}, b"logits overlaps X"),
        (dict(logits=DATA), {}, b"logits overlaps data"),
        (dict(logits=LABELS + 4), {}, b"logits overlaps labels"),
        (dict(correct=LOSS + N * 4 - 4), {}, b"loss overlaps correct"),
        (dict(loss=LOGITS + z_bytes - 4), {}, b"loss overlaps logits"),
        (dict(correct=LOGITS), {}, b"correct overlaps logits"),
        ({}, dict(ws=X + 256), b"workspace overlaps X"),
        ({}, dict(ws=DATA - need + 16), b"workspace overlaps data"),
        ({}, dict(ws=LABELS), b"workspace overlaps labels"),
        ({}, dict(ws=LOSS - need + 16), b"loss overlaps workspace"),
        ({}, dict(ws=CORRECT + 16), b"correct overlaps workspace"),
        ({}, dict(ws=LOGITS + z_bytes - 16 - (z_bytes - 16) % 16), b"logits overlaps workspace"),
    ]
    for kw, wkw, text in cases:
        rc, msg = call(valid(**kw), ws_bytes=need, **wkw)
        assert rc == INV and text in msg, (kw, wkw, msg)
    # exact extents: a shared test set ends after one agent's images and labels
    rc, msg = call(valid(s_data=0, loss=DATA + R * 3072 * 4 - 4), ws_bytes=need)
    assert rc == INV and b"loss overlaps data" in msg
    rc, msg = call(valid(s_labels=0, correct=LABELS + R * 4 - 4), ws_bytes=need)
    assert rc == INV and b"correct overlaps labels" in msg
    # touching is no overlap (tests/lenet_eval_sweep.cpp, where a call that passes launches
    # nothing); the plan query, which launches nothing either, accepts touching outputs
    rc, _, msg = plan(valid(correct=LOSS + N * 4, loss=LOSS, logits=LOSS + 2 * N * 4))
    assert rc == _lib.DL_OK, msg
    rc, _, msg = plan(valid(loss=X + x_bytes, correct=DATA - N * 4))
    assert rc == _lib.DL_OK, msg
    rc, _, msg = plan(valid(loss=X + x_bytes - 4))
    assert rc == INV and b"loss overlaps X" in msg


def test_sanitized_lenet_eval_sweep(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++", path="/opt/rocm/llvm/bin")
    if not cxx:
        pytest.skip("no host C++ compiler (g++ or the ROCm clang++)")
    exe = str(tmp_path / "lenet_eval_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "lenet_eval_sweep.cpp"),
                    os.path.join(CSRC, "launch.cpp"), os.path.join(CSRC, "plan.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr[:4000]
    out = run.stdout.split()
    assert out[1:] == ["calls,", "0", "failures"] and int(out[0]) >= 500
