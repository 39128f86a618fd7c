"""CPU checks of dl_lenet_grad's C ABI: the struct layout agrees between C and ctypes, the symbols
are additive (ABI still 10), the parameter count and ``BatchedLeNet.offsets`` are the header's
table and the ``LeNet`` module's, the workspace grows with each argument, every refusal the
header states comes back with its status and its own message before any device call (dummy
pointers, runs without a GPU), and the host-only shaping (csrc/launch.cpp shape_lenet) walks
every pass and group once inside a disjoint workspace, lists steps whose operands an earlier
step wrote and whose outputs stay inside their regions, and launches what
tests/golden/lenet_launches.txt pins -- the latter from tests/lenet_sweep.cpp, built with the
address and undefined-behaviour sanitizers and run as an ordinary process.

A line of the table reads
    name n_agents batch num_classes ldx_pad ldg_pad flags -> status n_launches steps
with ldx and ldg the parameter count rounded up to 4 plus the pad, ldz = num_classes + 2, s_logits
= batch * ldz + 5, s_data = batch * 3072, s_labels = batch + 1, and flags a comma list of g (G
given), loss, logits, nolabels, sdata0 and slab0 (a shared stride of 0).  The steps are, each after
the event e<k> recorded before it and the last followed by one more event,
    fwd grid {LenetConvArgs} | gemm {BgemmArgs} | head {launch_xent_grad's arguments} |
    bwd grid {LenetConvArgs} | reduce n_agents {LenetConvArgs}
with every field in declaration order and a pointer as its operand's name plus the byte offset
(X, DATA, LABELS, G, LOSS, LOGITS, WS).  The right sides were recorded at 256 compute units from
the commit before the step list: that commit's capi.hip, plan.cpp and launch.cpp linked against
recording stubs of launch_bgemm, launch_xent_grad, the three launch_lenet_conv_* functions and
hipEventRecord, run on the CPU over these left sides through dl_lenet_grad_events (and through
dl_lenet_grad, which launched the same without the events)."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-learning_amd", "csrc")

FIELDS = ["n_agents", "batch", "num_classes", "X", "ldx", "data", "s_data", "labels", "s_labels",
          "G", "ldg", "loss", "logits", "ldz", "s_logits"]
TABLE = {"conv1.weight": 0, "conv1.bias": 450, "conv2.weight": 456, "conv2.bias": 2856,
         "fc1.weight": 2872, "fc1.bias": 50872, "fc2.weight": 50992, "fc2.bias": 61072,
         "fc3.weight": 61156}


def test_struct_layout_matches_c(tmp_path):
    from distributed_learning_amd import _lib
    offs = "".join(f'printf("%zu ", offsetof(dl_lenet_args, {f}));' for f in FIELDS)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dlamd.h"\n'
                    'int main(void){printf("%zu ", sizeof(dl_lenet_args));' + offs +
                    'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                        check=True).stdout.split()]
    A = _lib.DlLenetArgs
    assert [f for f, _ in A._fields_] == FIELDS
    assert c == [ctypes.sizeof(A)] + [getattr(A, f).offset for f in FIELDS]


def test_symbols_are_additive():
    from distributed_learning_amd import _lib
    lib = _lib.load()
    for name in ("dl_lenet_param_count", "dl_lenet_workspace_bytes", "dl_lenet_grad",
                 "dl_lenet_grad_events"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.dl_abi_version() == 10 == _lib.ABI_VERSION


def test_param_count_and_offsets():
    from distributed_learning_amd import _lib
    from distributed_learning_amd.networks.batched_lenet import BatchedLeNet
    from distributed_learning_amd.networks.lenet import LeNet
    lib = _lib.load()
    assert lib.dl_lenet_param_count(10) == 62006
    assert lib.dl_lenet_param_count(0) == 0 and lib.dl_lenet_param_count(-3) == 0
    for nc in (1, 3, 10, 64):
        m = LeNet(nc)
        assert lib.dl_lenet_param_count(nc) == sum(p.numel() for p in m.parameters())
        named = [(k, tuple(p.shape)) for k, p in m.named_parameters()]
        assert named == LeNet.param_shapes(nc)
        b = BatchedLeNet(2, 4, nc, device="cpu")
        assert b.offsets == dict(TABLE, **{"fc3.bias": 61156 + 84 * nc})
        assert b.P == 61156 + 85 * nc == lib.dl_lenet_param_count(nc)
        assert (b.N, b.B, b.din, b.dout, b.path) == (2, 4, 3072, nc, "layers")
        assert b.loss.shape == (2,)
    for nc in (0, 65):
        with pytest.raises(ValueError, match="classes"):
            BatchedLeNet(2, 4, nc, device="cpu")


def test_workspace_grows_with_each_argument():
    from distributed_learning_amd import _lib
    ws = _lib.load().dl_lenet_workspace_bytes
    base = ws(4, 8, 10)
    assert base > 0 and base % 256 == 0
    assert ws(5, 8, 10) > base and ws(4, 9, 10) > base and ws(4, 8, 64) > base
    assert ws(4, 12, 10) > ws(4, 9, 10)                   # one more group of 4
    # at least what one agent-image keeps: pool1 + pool2 + the fc activations, in floats
    assert base >= 4 * 8 * (1176 + 400 + 2 * (120 + 84) + 400 + 2 * 10) * 4
    assert ws(0, 8, 10) == 0 and ws(4, 0, 10) == 0 and ws(4, 8, 0) == 0
    assert ws(65535, 1000, 64) > 2 ** 32                  # size_t, no 32-bit wrap


# dummy device addresses, never dereferenced, far apart
X, DATA, LABELS, G, LOSS, LOGITS, WS = (1 << 40, 1 << 44, 1 << 46, 1 << 48, 1 << 50, 1 << 51,
                                        1 << 52)
N, B, NC = 8, 64, 10
P = 62006
LD = 62016


def valid(**kw):
    from distributed_learning_amd import _lib
    a = _lib.DlLenetArgs(N, B, NC, X, LD, DATA, B * 3072, LABELS, B, G, LD, LOSS, LOGITS, 16,
                         B * 16)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def call(a, ws=WS, ws_bytes=None):
    """(status, message) of a call that must be refused before any device call."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    if ws_bytes is None:
        ws_bytes = lib.dl_lenet_workspace_bytes(max(a.n_agents, 1), max(a.batch, 1),
                                                min(max(a.num_classes, 1), 64)) if a else 0
    rc = lib.dl_lenet_grad(ctypes.byref(a) if a is not None else None, ws, ws_bytes, None)
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
    refused(valid(G=None, loss=None, logits=None), INV, b"no output")
    refused(valid(labels=None), INV, b"G and loss need labels")
    refused(valid(labels=None, G=None), INV, b"G and loss need labels")          # loss alone
    for f in ("n_agents", "batch"):
        for v in (0, -1):
            refused(valid(**{f: v}), INV, b"n_agents and batch must be >= 1")
    refused(valid(n_agents=65536), INV, b"at most 65535 agents")
    for nc in (0, -2):
        refused(valid(num_classes=nc), INV, b"num_classes must be >= 1")
    for nc in (65, 1000):
        refused(valid(num_classes=nc, ldx=1 << 20, ldg=1 << 20), UNS, b"at most 64 classes")
    for f, p in (("X", X), ("data", DATA), ("G", G)):
        for off in (4, 8):
            refused(valid(**{f: p + off}), INV, b"X, data and G must be 16-byte aligned")
    for ld in (P - 2, P + 1, LD + 2, 0, -LD):
        refused(valid(ldx=ld), INV, b"ldx must be a multiple of 4")
        refused(valid(ldg=ld), INV, b"ldg must be a multiple of 4")
    for sd in (B * 3072 - 4, B * 3072 + 2, 4, -B * 3072):
        refused(valid(s_data=sd), INV, b"s_data must be 0 (shared) or a multiple of 4")
    for sl in (B - 1, 1, -B):
        refused(valid(s_labels=sl), INV, b"s_labels must be 0 (shared) or >= batch")
    refused(valid(ldz=NC - 1), INV, b"logits need ldz >= num_classes")
    refused(valid(s_logits=(B - 1) * 16 + NC - 1), INV, b"logits need ldz >= num_classes")
    # the workspace: null, misaligned, one byte short
    need = _lib.load().dl_lenet_workspace_bytes(N, B, NC)
    refused(valid(), WSP, b"16-byte aligned workspace", ws=None)
    refused(valid(), WSP, b"16-byte aligned workspace", ws=WS + 4, ws_bytes=need + 4)
    refused(valid(), WSP, b"16-byte aligned workspace", ws_bytes=need - 1)
    assert len(seen) == 15                                  # each refusal has its own message
    # the messages are decided on the host: the forward-only and shared forms pass every check
    # up to the workspace, which is refused here so that nothing is launched
    for kw in (dict(G=None), dict(G=None, loss=None, labels=None), dict(s_data=0, s_labels=0),
               dict(logits=None), dict(ldx=P + 2, ldg=P + 2), dict(num_classes=64, ldz=64, ldx=66596,
                                                                   ldg=66600, s_logits=B * 64),
               dict(n_agents=65535, batch=1, s_data=3072, s_labels=1, s_logits=16)):
        rc, msg = call(valid(**kw), ws_bytes=0)
        assert rc == WSP, (kw, msg)


def test_overlap_refusals():
    from distributed_learning_amd import _lib
    INV = _lib.DL_ERR_INVALID
    need = _lib.load().dl_lenet_workspace_bytes(N, B, NC)
    x_bytes = ((N - 1) * LD + P) * 4
    d_bytes = N * B * 3072 * 4
    z_bytes = ((N - 1) * B * 16 + (B - 1) * 16 + NC) * 4
    cases = [
        (dict(G=X), {}, b"G overlaps X"),
        (dict(G=X + x_bytes - 8 - (x_bytes - 8) % 16), {}, b"G overlaps X"),
        (dict(G=DATA + d_bytes - 16), {}, b"G overlaps data"),
        (dict(G=LABELS), {}, b"G overlaps labels"),
        (dict(loss=X + 1024), {}, b"loss overlaps X"),
        (dict(loss=DATA + d_bytes - 4), {}, b"loss overlaps data"),
        (dict(loss=LABELS + N * B * 4 - 4), {}, b"loss overlaps labels"),
        (dict(logits=X + 64), {}, b"logits overlaps X"),
        (dict(logits=DATA), {}, b"logits overlaps data"),
        (dict(logits=LABELS + 4), {}, b"logits overlaps labels"),
        (dict(loss=G + 4096), {}, b"G overlaps loss"),
        (dict(logits=G + x_bytes - 4), {}, b"G overlaps logits"),
        (dict(loss=LOGITS + z_bytes - 4), {}, b"loss overlaps logits"),
        ({}, dict(ws=X + 256), b"workspace overlaps X"),
        ({}, dict(ws=DATA - need + 16), b"workspace overlaps data"),
        ({}, dict(ws=LABELS), b"workspace overlaps labels"),
        ({}, dict(ws=G - 256), b"G overlaps workspace"),
        ({}, dict(ws=LOSS - need + 16), b"loss overlaps workspace"),
        ({}, dict(ws=LOGITS + z_bytes - 16 - (z_bytes - 16) % 16), b"logits overlaps workspace"),
    ]
    for kw, wkw, text in cases:
        rc, msg = call(valid(**kw), ws_bytes=need, **wkw)
        assert rc == INV and text in msg, (kw, wkw, msg)
    # exact extents: a shared batch ends after one agent's images and labels
    rc, msg = call(valid(s_data=0, loss=DATA + B * 3072 * 4 - 4), ws_bytes=need)
    assert rc == INV and b"loss overlaps data" in msg
    rc, msg = call(valid(s_labels=0, loss=LABELS + B * 4 - 4), ws_bytes=need)
    assert rc == INV and b"loss overlaps labels" in msg
    # touching is no overlap (tests/lenet_sweep.cpp, where a call that passes launches nothing)


def test_sanitized_lenet_sweep(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++", path="/opt/rocm/llvm/bin")
    if not cxx:
        pytest.skip("no host C++ compiler (g++ or the ROCm clang++)")
    exe = str(tmp_path / "lenet_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "lenet_sweep.cpp"),
                    os.path.join(CSRC, "launch.cpp"), os.path.join(CSRC, "plan.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "lenet_launches.txt")],
                         capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr[:4000]
    # 180 calls of the grid and the 72 lines of the table
    assert run.stdout.split() == ["252", "calls,", "0", "failures"]
