"""CPU checks of the evaluation entry's C ABI (dl_mlp_eval, dl_mlp_eval_plan_query,
dl_mlp_eval_workspace_bytes): the struct layouts agree between C and ctypes, the grid shaping
follows the header's rule, and every refusal the header states comes back with its status and
message before any device call (dummy pointers, runs without a GPU).  Also dl_mlp_grad's and
dl_bgemm's checks on their own (csrc/launch.cpp shape_mlp_grad, check_bgemm) from
tests/mlp_sweep.cpp, built with the address and undefined-behaviour sanitizers and run as an
ordinary process."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARG_FIELDS = ["n_agents", "rows", "input_dim", "hidden_dim", "output_dim", "X", "ldx",
              "tile_cols", "data", "s_data", "labels", "s_labels", "loss", "correct", "logits",
              "ldz", "s_logits", "row_splits"]
PLAN_FIELDS = ["blocks", "row_splits", "grid", "lds_bytes"]


def test_struct_layout_matches_c(tmp_path):
    from distributed_learning_amd import _lib
    offs = "".join(f'printf("%zu ", offsetof(dl_mlp_eval_args, {f}));' for f in ARG_FIELDS)
    offs += "".join(f'printf("%zu ", offsetof(dl_mlp_eval_plan, {f}));' for f in PLAN_FIELDS)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dlamd.h"\n'
                    'int main(void){printf("%zu %zu ", sizeof(dl_mlp_eval_args), '
                    'sizeof(dl_mlp_eval_plan));' + offs + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                        check=True).stdout.split()]
    A, P = _lib.DlMlpEvalArgs, _lib.DlMlpEvalPlan
    assert [f for f, _ in A._fields_] == ARG_FIELDS and [f for f, _ in P._fields_] == PLAN_FIELDS
    py = [ctypes.sizeof(A), ctypes.sizeof(P)] + [getattr(A, f).offset for f in ARG_FIELDS] + \
        [getattr(P, f).offset for f in PLAN_FIELDS]
    assert c == py


def test_symbols_are_additive():
    from distributed_learning_amd import _lib
    lib = _lib.load()
    for name in ("dl_mlp_eval", "dl_mlp_eval_plan_query", "dl_mlp_eval_workspace_bytes"):
        assert hasattr(lib, name)
    assert lib.dl_abi_version() == 10


def test_workspace_bytes():
    from distributed_learning_amd import _lib
    ws = _lib.load().dl_mlp_eval_workspace_bytes
    assert ws(0, 100) == 0 and ws(-3, 100) == 0
    assert ws(256, 1) == ws(256, 64) > 0
    # [n_agents][blocks] float parts and as many int32 counts
    assert ws(256, 64) >= 256 * 1 * 8
    sizes = [ws(256, 64 * k) for k in (1, 2, 16, 156)]
    assert sizes == sorted(set(sizes))                     # grows with ceil(rows / 64)
    assert ws(256, 64 * 156 + 1) > ws(256, 64 * 156) >= 256 * 156 * 8
    assert ws(256, 64 * 16) % 16 == 0


# dummy device addresses, never dereferenced, far apart
X, DATA, LAB, LOSS, CORR, LOGITS, WS = (1 << 30, 1 << 34, 1 << 36, 1 << 37, 1 << 38, 1 << 40,
                                        1 << 44)
N, R, DIMS = 8, 200, (784, 150, 10)
P = 150 * 784 + 150 + 2 * (150 * 150 + 150) + 10 * 150 + 10


def valid(**kw):
    from distributed_learning_amd import _lib
    a = _lib.DlMlpEvalArgs(N, R, *DIMS, X, P, 0, DATA, 0, LAB, 0, LOSS, CORR, None, 0, 0, 0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def call(a, ws=WS, ws_bytes=1 << 20, plan_only=False):
    """(status, message, plan) of the plan query and, unless plan_only, of dl_mlp_eval with a
    good workspace too: they must agree."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    pl = _lib.DlMlpEvalPlan()
    ref = ctypes.byref(a) if a is not None else None
    rc = lib.dl_mlp_eval_plan_query(ref, ctypes.byref(pl))
    msg = lib.dl_last_error()
    if not plan_only:
        rc2 = lib.dl_mlp_eval(ref, ws, ws_bytes, None)
        assert rc2 == rc and lib.dl_last_error() == msg
    return rc, msg, pl


@pytest.mark.parametrize("rows,blocks", [(1, 1), (63, 1), (64, 1), (65, 2), (10000, 157)])
def test_plan_blocks_and_grid(rows, blocks):
    from distributed_learning_amd import _lib
    for n in (1, 8, 256, 1000):
        rc, msg, pl = call(valid(n_agents=n, rows=rows), plan_only=True)
        assert rc == _lib.DL_OK, msg
        assert pl.blocks == blocks and 1 <= pl.row_splits <= blocks
        assert pl.grid == n * pl.row_splits and 0 < pl.lds_bytes <= 160 * 1024
    # the caller's hint, clamped to [1, blocks]
    for hint, want in ((1000, blocks), (1, 1), (2, min(2, blocks))):
        rc, msg, pl = call(valid(rows=rows, row_splits=hint), plan_only=True)
        assert rc == _lib.DL_OK and pl.row_splits == want and pl.grid == N * want


def test_plan_covers_the_compute_units():
    """Few agents, many blocks: row splits until the workgroups cover the device's compute
    units (256 when no device is present), never more than the blocks."""
    from distributed_learning_amd import _lib
    rc, _, pl = call(valid(n_agents=4, rows=64 * 156), plan_only=True)
    assert rc == _lib.DL_OK and pl.row_splits > 1 and pl.grid >= 64
    rc, _, pl = call(valid(n_agents=4, rows=64 * 3), plan_only=True)
    assert rc == _lib.DL_OK and pl.row_splits == 3
    rc, _, pl = call(valid(n_agents=1000, rows=64 * 156), plan_only=True)
    assert rc == _lib.DL_OK and pl.row_splits == 1


def test_valid_variants():
    from distributed_learning_amd import _lib
    OK = _lib.DL_OK
    assert call(valid(), plan_only=True)[0] == OK
    assert call(valid(tile_cols=64, ldx=0), plan_only=True)[0] == OK           # tiled X
    assert call(valid(s_data=R * 784, s_labels=R), plan_only=True)[0] == OK    # per-agent sets
    assert call(valid(logits=LOGITS, ldz=13, s_logits=R * 13), plan_only=True)[0] == OK
    assert call(valid(labels=None, loss=None, correct=None, logits=LOGITS, ldz=10,
                      s_logits=R * 10), plan_only=True)[0] == OK               # logits only
    assert call(valid(loss=None), plan_only=True)[0] == OK
    assert call(valid(input_dim=16, hidden_dim=152, output_dim=16, ldx=1 << 16),
                plan_only=True)[0] == OK


def test_refusals():
    from distributed_learning_amd import _lib
    lib = _lib.load()
    INV, UNS = _lib.DL_ERR_INVALID, _lib.DL_ERR_UNSUPPORTED
    rc, msg, _ = call(None)
    assert rc == INV and b"args is NULL" in msg
    for f in ("X", "data"):
        rc, msg, _ = call(valid(**{f: None}))
        assert rc == INV and b"null X or data" in msg, (f, msg)
    rc, msg, _ = call(valid(labels=None))                      # loss given, no labels
    assert rc == INV and b"need labels" in msg
    rc, msg, _ = call(valid(labels=None, loss=None))           # correct given, no labels
    assert rc == INV and b"need labels" in msg
    for kw in (dict(input_dim=786), dict(hidden_dim=151), dict(hidden_dim=154),
               dict(output_dim=17), dict(rows=0)):
        rc, msg, _ = call(valid(ldx=1 << 20, **kw))
        assert rc == UNS and b"hidden_dim <= 152" in msg, (kw, msg)
    for s in (1, 4, R * 784 - 4, R * 784 - 1):
        rc, msg, _ = call(valid(s_data=s))
        assert rc == INV and b"s_data" in msg, (s, msg)
    rc, msg, _ = call(valid(s_data=R * 784 + 2))               # not a multiple of 4
    assert rc == INV and b"s_data" in msg
    rc, msg, _ = call(valid(s_labels=R - 1))
    assert rc == INV and b"s_labels" in msg
    rc, msg, _ = call(valid(logits=LOGITS, ldz=9, s_logits=R * 10))
    assert rc == INV and b"ldz" in msg
    rc, msg, _ = call(valid(logits=LOGITS, ldz=10, s_logits=R * 10 - 1))   # agents collide
    assert rc == INV and b"s_logits" in msg
    for off in (0, 4096, (N - 1) * P * 4):
        rc, msg, _ = call(valid(logits=X + off, ldz=10, s_logits=R * 10))
        assert rc == INV and b"overlaps X or data" in msg, off
    rc, msg, _ = call(valid(loss=DATA + 64))
    assert rc == INV and b"overlaps X or data" in msg
    rc, msg, _ = call(valid(correct=X + 4))
    assert rc == INV and b"overlaps X or data" in msg
    rc, msg, _ = call(valid(ldx=P - 4))
    assert rc == INV and b"bad arguments" in msg
    rc, msg, _ = call(valid(X=X + 4))
    assert rc == INV and b"16-byte aligned" in msg
    rc, msg, _ = call(valid(tile_cols=48, ldx=0))
    assert rc == INV and b"tile_cols" in msg
    rc, msg, _ = call(valid(n_agents=0))
    assert rc == INV and b"bad arguments" in msg
    # the tiled row must fit 32-bit offsets (dl_mlp_grad's limit)
    rc, msg, _ = call(valid(n_agents=20000, tile_cols=64, ldx=0))
    assert rc == UNS and b"32-bit" in msg
    a = valid()
    assert lib.dl_mlp_eval_plan_query(ctypes.byref(a), None) == INV


def test_workspace_refusals():
    from distributed_learning_amd import _lib
    lib = _lib.load()
    WSE = _lib.DL_ERR_WORKSPACE
    a = valid()
    need = lib.dl_mlp_eval_workspace_bytes(N, R)
    for ws, nbytes in ((None, need), (WS, need - 1), (WS, 0), (WS + 4, need + 64)):
        assert lib.dl_mlp_eval(ctypes.byref(a), ws, nbytes, None) == WSE, (ws, nbytes)
        assert b"workspace" in lib.dl_last_error()
    # a workspace on top of the inputs is an argument error
    assert lib.dl_mlp_eval(ctypes.byref(a), X, need, None) == _lib.DL_ERR_INVALID
    assert b"workspace overlaps" in lib.dl_last_error()
    # argument refusals come first, whatever the workspace
    assert lib.dl_mlp_eval(ctypes.byref(valid(hidden_dim=151)), None, 0, None) == \
        _lib.DL_ERR_UNSUPPORTED


def test_sanitized_mlp_sweep(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++", path="/opt/rocm/llvm/bin")
    if not cxx:
        pytest.skip("no host C++ compiler (g++ or the ROCm clang++)")
    csrc = os.path.join(ROOT, "distributed-learning_amd", "csrc")
    exe = str(tmp_path / "mlp_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "mlp_sweep.cpp"),
                    os.path.join(csrc, "launch.cpp"), os.path.join(csrc, "plan.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr[:4000]
    assert run.stdout.split() == ["91", "calls,", "0", "failures"]
