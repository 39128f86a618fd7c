"""CPU checks of the fused momentum round's C ABI (dl_sgd_round, dl_sgd_round_plan): the struct
layout agrees between C and ctypes, and every refusal the header states comes back with its
status and message before any device call (runs without a GPU)."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layout_matches_c(tmp_path):
    from distributed_learning_amd import _lib
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dlamd.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n",'
                    'sizeof(dl_sgd_round_args), offsetof(dl_sgd_round_args, buf),'
                    'offsetof(dl_sgd_round_args, ldb), offsetof(dl_sgd_round_args, momentum),'
                    'offsetof(dl_sgd_round_args, weight_decay),'
                    'offsetof(dl_sgd_round_args, nesterov), offsetof(dl_sgd_round_args, first));'
                    'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                        check=True).stdout.split()]
    A = _lib.DlSgdRoundArgs
    py = [ctypes.sizeof(A), A.buf.offset, A.ldb.offset, A.momentum.offset, A.weight_decay.offset,
          A.nesterov.offset, A.first.offset]
    assert c == py
    assert A.mix.offset == 0 and A.buf.offset == ctypes.sizeof(_lib.DlMixArgs)


def test_symbols_are_additive():
    """New symbols, the ABI version unchanged: callers detect the fused round by the symbol."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "dl_sgd_round") and hasattr(lib, "dl_sgd_round_plan")
    assert lib.dl_abi_version() == 10


# dummy device addresses, never dereferenced: 64 agents x 4096 params, far apart
X, Y, G, B = 1 << 30, 1 << 32, 1 << 34, 1 << 36
N, P = 64, 4096
BYTES = N * P * 4


def valid(**kw):
    from distributed_learning_amd import _lib
    a = _lib.DlSgdRoundArgs()
    m = a.mix
    m.x, m.y, m.g = X, Y, G
    m.ldx = m.ldy = m.ldg = P
    m.n_params = P
    m.lr = 0.1
    m.W = _lib.DlCsr(1 << 20, 1 << 21, 1 << 22, N, 5 * N, 5, 0, 0, 5)
    a.buf, a.ldb = B, P
    a.momentum, a.weight_decay = 0.9, 5e-4
    for k, v in kw.items():
        if k.startswith("mix_"):
            setattr(a.mix, k[4:], v)
        else:
            setattr(a, k, v)
    return a


def call(a, plan_only=False):
    """(status, message) of dl_sgd_round_plan and, unless plan_only, of dl_sgd_round too (they
    must agree)."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    pl = _lib.DlMixPlan()
    ref = ctypes.byref(a) if a is not None else None
    rc = lib.dl_sgd_round_plan(ref, ctypes.byref(pl))
    msg = lib.dl_last_error()
    if not plan_only:
        rc2 = lib.dl_sgd_round(ref, None, 0, None)
        assert rc2 == rc and lib.dl_last_error() == msg
    return rc, msg, pl


def test_valid_arguments_plan_path_1():
    from distributed_learning_amd import _lib
    rc, msg, pl = call(valid(), plan_only=True)
    assert rc == _lib.DL_OK, msg
    assert pl.path == 1 and pl.tile_cols > 0 and pl.grid > 0 and pl.n_tiles * pl.tile_cols == P
    # the same plan as the plain round's on the same dl_mix_args (one planner)
    a = valid()
    pm = _lib.DlMixPlan()
    assert _lib.load().dl_mix_plan_query(ctypes.byref(a.mix), ctypes.byref(pm)) == _lib.DL_OK
    assert [getattr(pl, f) for f, _ in pl._fields_] == [getattr(pm, f) for f, _ in pm._fields_]
    # in place (y == x, ldy == ldx), momentum 0 without a buffer, the column-tiled layout
    assert call(valid(mix_y=X), plan_only=True)[0] == _lib.DL_OK
    assert call(valid(momentum=0.0, buf=None, ldb=0), plan_only=True)[0] == _lib.DL_OK
    t = dict(mix_tile_cols=64, mix_ldx=0, mix_ldy=0, mix_ldg=0, ldb=0)
    assert call(valid(**t), plan_only=True)[0] == _lib.DL_OK
    assert call(valid(mix_y=X, **t), plan_only=True)[0] == _lib.DL_OK


def test_invalid_arguments():
    from distributed_learning_amd import _lib
    lib = _lib.load()
    INV = _lib.DL_ERR_INVALID
    assert call(None)[0] == INV
    for f in ("mix_x", "mix_y", "mix_g"):
        rc, msg, _ = call(valid(**{f: None}))
        assert rc == INV and b"null x/y/g" in msg, (f, msg)
    rc, msg, _ = call(valid(buf=None))                       # momentum without a buffer
    assert rc == INV and b"momentum" in msg
    rc, msg, _ = call(valid(ldb=P - 1))                      # ... or with ldb < n_params
    assert rc == INV and b"momentum" in msg
    rc, msg, _ = call(valid(mix_tile_cols=64, mix_ldx=0, mix_ldy=0, mix_ldg=0, ldb=N - 1))
    assert rc == INV and b"momentum" in msg                  # tiled: block rows < n_rows
    rc, msg, _ = call(valid(nesterov=1, momentum=0.0, buf=None))
    assert rc == INV and b"Nesterov" in msg
    rc, msg, _ = call(valid(nesterov=1, momentum=-0.5))
    assert rc == INV and b"Nesterov" in msg
    rc, msg, _ = call(valid(nesterov=1, dampening=0.1))
    assert rc == INV and b"Nesterov" in msg
    # y overlapping x other than y == x with ldy == ldx
    rc, msg, _ = call(valid(mix_y=X + 64))
    assert rc == INV and b"y overlaps x" in msg
    rc, msg, _ = call(valid(mix_y=X, mix_ldy=P + 4))
    assert rc == INV and b"y overlaps x" in msg
    rc, msg, _ = call(valid(mix_y=X + BYTES - 4))
    assert rc == INV and b"y overlaps x" in msg
    # buf overlapping x, y or g (in place too)
    for base in (X, Y, G):
        for off in (0, 4096, BYTES - 4, -(BYTES - 4)):
            rc, msg, _ = call(valid(buf=base + off))
            assert rc == INV and b"buf overlaps" in msg, (base, off, msg)
    rc, msg, _ = call(valid(mix_y=X, buf=X))
    assert rc == INV and b"buf overlaps" in msg
    assert call(valid(buf=X + BYTES), plan_only=True)[0] == _lib.DL_OK   # adjacent: fine
    # g overlapping the output of an in-place round
    rc, msg, _ = call(valid(mix_y=X, mix_g=X + 4096))
    assert rc == INV and b"overlaps g" in msg
    # the plain round's own checks still apply (the texts say dl_mix_round)
    rc, msg, _ = call(valid(mix_n_params=0))
    assert rc == INV and b"n_params" in msg
    # plan pointer
    a = valid()
    assert lib.dl_sgd_round_plan(ctypes.byref(a), None) == INV
    # the plain round still refuses y == x
    assert lib.dl_mix_round(ctypes.byref(valid(mix_y=X).mix), None, 0, None) == INV
    assert b"y overlaps x" in lib.dl_last_error()


def test_unsupported_arguments(monkeypatch):
    from distributed_learning_amd import _lib
    UNS = _lib.DL_ERR_UNSUPPORTED
    n_parts = ctypes.c_int32(0)
    rows = (ctypes.c_int32 * 1)(4)
    for kw in (dict(mix_halo=1 << 38), dict(mix_n_halo=4), dict(mix_halo=1 << 38, mix_n_halo=4,
                                                                mix_ldh=P),
               dict(mix_mean_prev=1 << 38), dict(mix_colsum_out=1 << 38),
               dict(mix_n_local_src=N), dict(mix_n_local_src=N + 8),
               dict(mix_n_halo_blocks=1, mix_halo_block_rows=ctypes.cast(rows, ctypes.c_void_p)),
               dict(mix_partial_rows_out=ctypes.pointer(n_parts))):
        rc, msg, _ = call(valid(**kw))
        assert rc == UNS and b"halo" in msg, (kw, msg)
    # a plan path other than 1: the gather path (forced) ...
    monkeypatch.setenv("DLAMD_FORCE_GATHER", "1")
    rc, msg, _ = call(valid())
    assert rc == UNS and b"path 2" in msg
    monkeypatch.delenv("DLAMD_FORCE_GATHER")
    # ... and the register-CSR paths: 4096 agents with per-edge weights (path 4), an irregular
    # graph of 3000 agents (path 5)
    from distributed_learning_amd import _lib as L
    big = dict(mix_ldx=1 << 16, mix_ldy=1 << 16, mix_ldg=1 << 16, ldb=1 << 16,
               mix_n_params=1 << 16, mix_x=1 << 40, mix_y=1 << 42, mix_g=1 << 44, buf=1 << 46)
    rc, msg, _ = call(valid(mix_W=L.DlCsr(1 << 20, 1 << 21, 1 << 22, 4096, 5 * 4096, 5, 0, 0, 5),
                            **big))
    assert rc == UNS and b"path 4" in msg
    rc, msg, _ = call(valid(mix_W=L.DlCsr(1 << 20, 1 << 21, 1 << 22, 3000, 9000, 0, 1, 0, 3),
                            **big))
    assert rc == UNS and b"path 5" in msg
