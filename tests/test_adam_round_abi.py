"""CPU checks of Adam's C ABI (dl_adam_round, dl_adam_round_plan, dl_adam_step, dl_adam_tick):
the struct layouts agree between C and ctypes, and every refusal the header states comes back
with its status and message before any device call (runs without a GPU)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND_FIELDS = ("m", "ldm", "v", "ldv", "beta1", "beta2", "eps", "weight_decay", "decoupled",
                "step_size", "bias2_sqrt", "coef")
STEP_FIELDS = ("x", "ldx", "g", "ldg", "m", "ldm", "v", "ldv", "out", "ldo", "n_rows", "n_params",
               "beta1", "beta2", "lr", "eps", "weight_decay", "decoupled", "step_size",
               "bias2_sqrt", "coef")


@pytest.mark.parametrize("struct,cls,fields", [("dl_adam_round_args", "DlAdamRoundArgs",
                                                ROUND_FIELDS),
                                               ("dl_adam_args", "DlAdamArgs", STEP_FIELDS)])
def test_struct_layout_matches_c(tmp_path, struct, cls, fields):
    from distributed_learning_amd import _lib
    prog = tmp_path / "layout.c"
    offs = ",".join(f"offsetof({struct}, {f})" for f in fields)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dlamd.h"\n'
                    'int main(void){printf("' + "%zu " * (len(fields) + 1) + '\\n",'
                    f'sizeof({struct}),' + offs + ');return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                        check=True).stdout.split()]
    A = getattr(_lib, cls)
    assert c == [ctypes.sizeof(A)] + [getattr(A, f).offset for f in fields]
    if cls == "DlAdamRoundArgs":
        assert A.mix.offset == 0 and A.m.offset == ctypes.sizeof(_lib.DlMixArgs)


def test_state_layout_matches_c(tmp_path):
    from distributed_learning_amd import _lib
    names = ("T", "B1T", "B2T", "LR", "BETA1", "BETA2", "COEF", "STATE_LEN")
    prog = tmp_path / "state.c"
    prog.write_text('#include <stdio.h>\n#include "dlamd.h"\nint main(void){printf("'
                    + "%d " * len(names) + '\\n",' + ",".join("DL_ADAM_" + n for n in names)
                    + ');return 0;}\n')
    exe = tmp_path / "state"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                        check=True).stdout.split()]
    assert c == [_lib.ADAM_T, _lib.ADAM_B1T, _lib.ADAM_B2T, _lib.ADAM_LR, _lib.ADAM_BETA1,
                 _lib.ADAM_BETA2, _lib.ADAM_COEF, _lib.ADAM_STATE_LEN] == [0, 1, 2, 3, 4, 5, 6, 8]


def test_symbols_are_additive():
    """New symbols, the ABI version unchanged: callers detect Adam by the symbols."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    for name in ("dl_adam_round", "dl_adam_round_plan", "dl_adam_step", "dl_adam_tick"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.dl_abi_version() == 10 and _lib.ABI_VERSION == 10


# dummy device addresses, never dereferenced: 64 agents x 4096 params, far apart
X, Y, G, M, V, C = 1 << 30, 1 << 32, 1 << 34, 1 << 36, 1 << 37, 1 << 38
N, P = 64, 4096
BYTES = N * P * 4
TILED = dict(mix_tile_cols=64, mix_ldx=0, mix_ldy=0, mix_ldg=0, ldm=0, ldv=0)
INF, NAN = float("inf"), float("nan")


def valid(**kw):
    from distributed_learning_amd import _lib
    a = _lib.DlAdamRoundArgs()
    m = a.mix
    m.x, m.y, m.g = X, Y, G
    m.ldx = m.ldy = m.ldg = P
    m.n_params = P
    m.lr = 0.001
    m.W = _lib.DlCsr(1 << 20, 1 << 21, 1 << 22, N, 5 * N, 5, 1, 1, 5)
    a.m, a.v = M, V
    a.ldm = a.ldv = P
    a.beta1, a.beta2, a.eps = 0.9, 0.999, 1e-8
    a.step_size, a.bias2_sqrt = 0.01, 0.0316
    for k, v in kw.items():
        if k.startswith("mix_"):
            setattr(a.mix, k[4:], v)
        else:
            setattr(a, k, v)
    return a


def call(a, plan_only=False):
    """(status, message, plan) of dl_adam_round_plan and, unless plan_only, of dl_adam_round too
    (they must agree)."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    pl = _lib.DlMixPlan()
    ref = ctypes.byref(a) if a is not None else None
    rc = lib.dl_adam_round_plan(ref, ctypes.byref(pl))
    msg = lib.dl_last_error()
    if not plan_only:
        rc2 = lib.dl_adam_round(ref, None, 0, None)
        assert rc2 == rc and lib.dl_last_error() == msg
    return rc, msg, pl


def test_valid_arguments_plan_path_1():
    from distributed_learning_amd import _lib
    rc, msg, pl = call(valid(), plan_only=True)
    assert rc == _lib.DL_OK, msg
    assert pl.path == 1 and pl.tile_cols > 0 and pl.grid > 0 and pl.n_tiles * pl.tile_cols == P
    # the same plan as the plain round's on the same dl_mix_args (one planner)
    for kw in ({}, TILED, dict(mix_dev_sq=1 << 40, mix_dev_max=1 << 41)):
        a = valid(**kw)
        pm = _lib.DlMixPlan()
        assert _lib.load().dl_mix_plan_query(ctypes.byref(a.mix), ctypes.byref(pm)) == _lib.DL_OK
        rc, msg, pl = call(a, plan_only=True)
        assert rc == _lib.DL_OK, msg
        assert [getattr(pl, f) for f, _ in pl._fields_] == [getattr(pm, f) for f, _ in pm._fields_]
    # x' = x is accepted, row-major and column-tiled; so are both optimizers, the device
    # coefficients (the by-value ones then ignored), beta 0 and eps 0
    for kw in (dict(mix_y=X), dict(weight_decay=5e-4), dict(weight_decay=1e-2, decoupled=1),
               dict(coef=C, step_size=NAN, bias2_sqrt=INF), dict(beta1=0.0, beta2=0.0),
               dict(eps=0.0)):
        assert call(valid(**kw), plan_only=True)[0] == _lib.DL_OK, kw
        assert call(valid(**kw, **TILED), plan_only=True)[0] == _lib.DL_OK, kw
    # padded rows: every stride its own
    assert call(valid(mix_ldx=P + 4, mix_ldy=P + 8, mix_ldg=P + 12, ldm=P + 16, ldv=P + 20),
                plan_only=True)[0] == _lib.DL_OK
    # the workspace rule: a deviation without a workspace is the round's DL_ERR_WORKSPACE, as
    # dl_mix_round's; the plan query has no workspace to refuse
    a = valid(mix_dev_sq=1 << 40, mix_dev_max=1 << 41)
    lib = _lib.load()
    assert lib.dl_adam_round_plan(ctypes.byref(a), ctypes.byref(pl)) == _lib.DL_OK
    assert lib.dl_adam_round(ctypes.byref(a), None, 0, None) == _lib.DL_ERR_WORKSPACE
    assert b"workspace" in lib.dl_last_error()
    assert lib.dl_adam_round(ctypes.byref(a), 1 << 42, 16, None) == _lib.DL_ERR_WORKSPACE
    assert b"workspace" in lib.dl_last_error()
    assert lib.dl_adam_round(ctypes.byref(a), (1 << 42) + 4, 1 << 24, None) == \
        _lib.DL_ERR_WORKSPACE                                   # not 16-byte aligned


def test_invalid_arguments():
    from distributed_learning_amd import _lib
    lib = _lib.load()
    INV = _lib.DL_ERR_INVALID
    rc, msg, _ = call(None)
    assert rc == INV and b"args is NULL" in msg
    for f in ("mix_x", "mix_y", "mix_g", "m", "v"):
        rc, msg, _ = call(valid(**{f: None}))
        assert rc == INV and b"dl_adam_round: null x/y/g/m/v" in msg, (f, msg)
    # everything dl_mix_round refuses (the texts say dl_mix_round)
    rc, msg, _ = call(valid(mix_W=_lib.DlCsr(None, 1 << 21, 1 << 22, N, 5 * N, 5, 1, 1, 5)))
    assert rc == INV and b"null x/y/row_ptr/col/w" in msg
    rc, msg, _ = call(valid(mix_ldx=P - 1))
    assert rc == INV and b"ldx/ldy smaller than n_params" in msg
    rc, msg, _ = call(valid(mix_ldg=P - 1))
    assert rc == INV and b"ldg < n_params" in msg
    rc, msg, _ = call(valid(mix_n_params=0))
    assert rc == INV and b"n_params" in msg
    rc, msg, _ = call(valid(**{**TILED, "mix_tile_cols": 48}))
    assert rc == INV and b"tile_cols" in msg
    # a moment not laid out as x
    for f in ("ldm", "ldv"):
        rc, msg, _ = call(valid(**{f: P - 1}))
        assert rc == INV and b"dl_adam_round: m and v laid out as x" in msg, (f, msg)
        for v in (N - 1, -1):                                      # tiled: block rows < n_rows
            rc, msg, _ = call(valid(**{**TILED, f: v}))
            assert rc == INV and b"dl_adam_round: m and v laid out as x" in msg, (f, v, msg)
    # the optimizer's parameters
    for f in ("beta1", "beta2"):
        for b in (-0.1, 1.0, 1.5, NAN, INF):
            rc, msg, _ = call(valid(**{f: b}))
            assert rc == INV and b"dl_adam_round: beta1 and beta2 must be in [0, 1)" in msg, (f, b)
    for e in (-1e-8, NAN):
        rc, msg, _ = call(valid(eps=e))
        assert rc == INV and b"dl_adam_round: eps must be >= 0" in msg, e
    for f in ("step_size", "bias2_sqrt"):
        for c in (INF, -INF, NAN):
            rc, msg, _ = call(valid(**{f: c}))
            assert rc == INV and b"step_size and bias2_sqrt must be finite when coef is NULL" \
                in msg, (f, c, msg)
    # alignment the round refuses: column-tiled operands off 16 bytes, from the round itself --
    # the plan query stops before
    for kw in (dict(mix_x=X + 4), dict(mix_g=G + 4), dict(m=M + 4), dict(v=V + 4)):
        a = valid(**kw, **TILED)
        assert lib.dl_adam_round(ctypes.byref(a), None, 0, None) == INV, kw
        assert b"tiled operands must be 16-byte aligned" in lib.dl_last_error()
    # m or v overlapping x, y or g in any way, or each other
    for mom, other in (("m", V), ("v", M)):
        for name, base in (("x", X), ("y", Y), ("g", G)):
            for off in (0, 64, BYTES - 4, -BYTES + 4):
                rc, msg, _ = call(valid(**{mom: base + off}))
                want = f"dl_adam_round: {mom} overlaps {name}".encode()
                assert rc == INV and want in msg, (mom, name, off, msg)
        for off in (0, 64, BYTES - 4, -BYTES + 4):
            rc, msg, _ = call(valid(**{mom: other + off}))
            assert rc == INV and b"dl_adam_round: m overlaps v" in msg, (mom, off, msg)
    rc, msg, _ = call(valid(m=X, mix_y=X))                             # m on the in-place x
    assert rc == INV and b"dl_adam_round: m overlaps x" in msg
    rc, msg, _ = call(valid(v=M + 64 * 4 * N, **TILED))                # one tile into m
    assert rc == INV and b"dl_adam_round: m overlaps v" in msg
    # y overlapping g (the plain round's text), and x other than y == x with ldy == ldx
    for off in (0, 64, BYTES - 4):
        rc, msg, _ = call(valid(mix_y=G + off))
        assert rc == INV and b"y overlaps g" in msg
    for kw in (dict(mix_y=X + 64), dict(mix_y=X, mix_ldy=P + 4), dict(mix_y=X + BYTES - 4),
               dict(mix_y=X - BYTES + 4)):
        rc, msg, _ = call(valid(**kw))
        assert rc == INV and b"y overlaps x" in msg, (kw, msg)
    assert call(valid(m=M + BYTES, mix_y=X + BYTES), plan_only=True)[0] == _lib.DL_OK  # adjacent
    # plan pointer
    a = valid()
    assert lib.dl_adam_round_plan(ctypes.byref(a), None) == INV
    assert b"plan is NULL" in lib.dl_last_error()


def test_unsupported_arguments(monkeypatch):
    from distributed_learning_amd import _lib
    UNS = _lib.DL_ERR_UNSUPPORTED
    n_parts = ctypes.c_int32(0)
    rows = (ctypes.c_int32 * 1)(4)
    for kw in (dict(mix_halo=1 << 40), dict(mix_n_halo=4), dict(mix_halo=1 << 40, mix_n_halo=4,
                                                                mix_ldh=P),
               dict(mix_mean_prev=1 << 40), dict(mix_colsum_out=1 << 40),
               dict(mix_n_local_src=N), dict(mix_n_local_src=N + 8),
               dict(mix_n_halo_blocks=1, mix_halo_block_rows=ctypes.cast(rows, ctypes.c_void_p)),
               dict(mix_partial_rows_out=ctypes.pointer(n_parts))):
        rc, msg, _ = call(valid(**kw))
        assert rc == UNS and b"dl_adam_round: no halo rows, partition row sets or lagged " \
            b"deviation" in msg, (kw, msg)
    # a plan path other than 1: the gather path (forced) ...
    monkeypatch.setenv("DLAMD_FORCE_GATHER", "1")
    rc, msg, _ = call(valid())
    assert rc == UNS and b"dl_adam_round: the fused Adam round runs on the LDS tile kernel " \
        b"(plan path 1); this round plans path 2" in msg
    monkeypatch.delenv("DLAMD_FORCE_GATHER")
    # ... and the register-CSR paths: 4096 agents with per-edge weights (path 4), an irregular
    # graph of 3000 agents (path 5)
    ld = 1 << 16
    big = dict(mix_ldx=ld, mix_ldy=ld, mix_ldg=ld, ldm=ld, ldv=ld, mix_n_params=ld,
               mix_x=1 << 40, mix_y=1 << 42, mix_g=1 << 44, m=1 << 46, v=1 << 48)
    rc, msg, _ = call(valid(mix_W=_lib.DlCsr(1 << 20, 1 << 21, 1 << 22, 4096, 5 * 4096, 5, 0, 0, 5),
                            **big))
    assert rc == UNS and b"this round plans path 4" in msg
    rc, msg, _ = call(valid(mix_W=_lib.DlCsr(1 << 20, 1 << 21, 1 << 22, 3000, 9000, 0, 1, 0, 3),
                            **big))
    assert rc == UNS and b"this round plans path 5" in msg
    # ... the forced register-CSR path in the column-tiled layout, in place
    monkeypatch.setenv("DLAMD_FORCE_REG", "1")
    t = dict(TILED, mix_tile_cols=4, mix_n_params=64, mix_y=X)
    rc, msg, _ = call(valid(mix_W=_lib.DlCsr(1 << 20, 1 << 21, 1 << 22, 1500, 7500, 5, 1, 1, 5),
                            **t))
    assert rc == UNS and b"this round plans path 4" in msg


def step_args(**kw):
    from distributed_learning_amd import _lib
    a = _lib.DlAdamArgs(X, P, G, P, M, P, V, P, Y, P, N, P, 0.9, 0.999, 1e-3, 1e-8, 0.0, 0, 0.01,
                        0.0316, None)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_step_and_tick_refusals():
    """dl_adam_step's and dl_adam_tick's refusals, each before any device call."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    INV = _lib.DL_ERR_INVALID

    def step(**kw):
        rc = lib.dl_adam_step(ctypes.byref(step_args(**kw)), None)
        return rc, lib.dl_last_error()
    assert lib.dl_adam_step(None, None) == INV and b"null args" in lib.dl_last_error()
    # nothing to do: no launch, no check
    assert step(n_rows=0)[0] == _lib.DL_OK and step(n_params=0)[0] == _lib.DL_OK
    for kw in (dict(x=None), dict(g=None), dict(m=None), dict(v=None), dict(out=None),
               dict(ldx=P - 1), dict(ldg=P - 1), dict(ldm=P - 1), dict(ldv=P - 1),
               dict(ldo=P - 1), dict(n_rows=65536), dict(n_rows=-1)):
        rc, msg = step(**kw)
        assert rc == INV and b"dl_adam_step: bad arguments" in msg, (kw, msg)
    for kw, text in ((dict(beta1=1.0), b"beta1 and beta2 must be in [0, 1)"),
                     (dict(beta2=-0.5), b"beta1 and beta2 must be in [0, 1)"),
                     (dict(eps=-1.0), b"eps must be >= 0"),
                     (dict(step_size=INF), b"must be finite when coef is NULL"),
                     (dict(bias2_sqrt=NAN), b"must be finite when coef is NULL"),
                     (dict(out=X + 64), b"out must be x itself or not overlap it"),
                     (dict(m=X), b"m overlaps x"), (dict(m=G + 64), b"m overlaps g"),
                     (dict(m=Y + BYTES - 4), b"m overlaps out"), (dict(v=X), b"v overlaps x"),
                     (dict(v=G), b"v overlaps g"), (dict(v=Y), b"v overlaps out"),
                     (dict(v=M + 64), b"m overlaps v"), (dict(out=X, v=X), b"v overlaps x")):
        rc, msg = step(**kw)
        assert rc == INV and b"dl_adam_step: " in msg and text in msg, (kw, msg)
    assert lib.dl_adam_tick(None, None) == INV and b"dl_adam_tick: state" in lib.dl_last_error()
    assert lib.dl_adam_tick(ctypes.c_void_p((1 << 30) + 4), None) == INV
