"""CPU checks of the Chebyshev round's C ABI (dl_cheb_round, dl_cheb_round_plan, dl_axpby): the
struct layout agrees between C and ctypes, and every refusal the header states comes back with
its status and message before any device call (runs without a GPU)."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layout_matches_c(tmp_path):
    from distributed_learning_amd import _lib
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dlamd.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu\\n",'
                    'sizeof(dl_cheb_round_args), offsetof(dl_cheb_round_args, z),'
                    'offsetof(dl_cheb_round_args, ldz), offsetof(dl_cheb_round_args, a),'
                    'offsetof(dl_cheb_round_args, b));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                        check=True).stdout.split()]
    A = _lib.DlChebRoundArgs
    assert c == [ctypes.sizeof(A), A.z.offset, A.ldz.offset, A.a.offset, A.b.offset]
    assert A.mix.offset == 0 and A.z.offset == ctypes.sizeof(_lib.DlMixArgs)


def test_symbols_are_additive():
    """New symbols, the ABI version unchanged: callers detect the round by the symbol."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    for name in ("dl_cheb_round", "dl_cheb_round_plan", "dl_axpby"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.dl_abi_version() == 10 and _lib.ABI_VERSION == 10


# dummy device addresses, never dereferenced: 64 agents x 4096 params, far apart
X, Y, Z, G = 1 << 30, 1 << 32, 1 << 34, 1 << 36
N, P = 64, 4096
BYTES = N * P * 4
TILED = dict(mix_tile_cols=64, mix_ldx=0, mix_ldy=0, ldz=0)


def valid(**kw):
    from distributed_learning_amd import _lib
    a = _lib.DlChebRoundArgs()
    m = a.mix
    m.x, m.y = X, Y
    m.ldx = m.ldy = P
    m.n_params = P
    m.W = _lib.DlCsr(1 << 20, 1 << 21, 1 << 22, N, 5 * N, 5, 1, 1, 5)
    a.z, a.ldz = Z, P
    a.a, a.b = 1.5, -0.5
    for k, v in kw.items():
        if k.startswith("mix_"):
            setattr(a.mix, k[4:], v)
        else:
            setattr(a, k, v)
    return a


def call(a, plan_only=False):
    """(status, message, plan) of dl_cheb_round_plan and, unless plan_only, of dl_cheb_round too
    (they must agree)."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    pl = _lib.DlMixPlan()
    ref = ctypes.byref(a) if a is not None else None
    rc = lib.dl_cheb_round_plan(ref, ctypes.byref(pl))
    msg = lib.dl_last_error()
    if not plan_only:
        rc2 = lib.dl_cheb_round(ref, None, 0, None)
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
    # y == z (the intended mode) and y == x are accepted, row-major and column-tiled; so is z == x
    for kw in (dict(mix_y=Z), dict(mix_y=X), dict(z=X), dict(z=X, mix_y=X)):
        assert call(valid(**kw), plan_only=True)[0] == _lib.DL_OK, kw
        assert call(valid(**kw, **TILED), plan_only=True)[0] == _lib.DL_OK, kw
    assert call(valid(**TILED), plan_only=True)[0] == _lib.DL_OK
    # padded rows: every stride its own
    assert call(valid(mix_ldx=P + 4, mix_ldy=P + 8, ldz=P + 12), plan_only=True)[0] == _lib.DL_OK
    # a deviation without a workspace is the round's DL_ERR_WORKSPACE, as dl_mix_round's; the plan
    # query has no workspace to refuse
    a = valid(mix_dev_sq=1 << 38, mix_dev_max=1 << 39)
    lib = _lib.load()
    assert lib.dl_cheb_round_plan(ctypes.byref(a), ctypes.byref(pl)) == _lib.DL_OK
    assert lib.dl_cheb_round(ctypes.byref(a), None, 0, None) == _lib.DL_ERR_WORKSPACE
    assert b"workspace" in lib.dl_last_error()
    assert lib.dl_cheb_round(ctypes.byref(a), 1 << 40, 16, None) == _lib.DL_ERR_WORKSPACE
    assert b"workspace" in lib.dl_last_error()


def test_invalid_arguments():
    from distributed_learning_amd import _lib
    lib = _lib.load()
    INV = _lib.DL_ERR_INVALID
    rc, msg, _ = call(None)
    assert rc == INV and b"args is NULL" in msg
    for f in ("mix_x", "mix_y", "z"):
        rc, msg, _ = call(valid(**{f: None}))
        assert rc == INV and b"null x/y/z" in msg, (f, msg)
    rc, msg, _ = call(valid(mix_W=_lib.DlCsr(None, 1 << 21, 1 << 22, N, 5 * N, 5, 1, 1, 5)))
    assert rc == INV and b"null x/y/row_ptr/col/w" in msg           # W's arrays
    rc, msg, _ = call(valid(mix_g=G, mix_ldg=P))                      # no gradient term
    assert rc == INV and b"g must be NULL" in msg
    # strides the round itself refuses (the texts say dl_mix_round), and z's
    rc, msg, _ = call(valid(mix_ldx=P - 1))
    assert rc == INV and b"ldx/ldy smaller than n_params" in msg
    rc, msg, _ = call(valid(mix_n_params=0))
    assert rc == INV and b"n_params" in msg
    rc, msg, _ = call(valid(mix_tile_cols=48, mix_ldx=0, mix_ldy=0, ldz=0))
    assert rc == INV and b"tile_cols" in msg
    rc, msg, _ = call(valid(ldz=P - 1))
    assert rc == INV and b"z laid out as x" in msg
    rc, msg, _ = call(valid(**{**TILED, "ldz": N - 1}))               # tiled: block rows < n_rows
    assert rc == INV and b"z laid out as x" in msg
    rc, msg, _ = call(valid(**{**TILED, "ldz": -1}))
    assert rc == INV and b"z laid out as x" in msg
    # alignment the round refuses: column-tiled operands off 16 bytes (x by the plain round's
    # check, z by the Chebyshev round's), from the round itself -- the plan query stops before
    for kw in (dict(mix_x=X + 4), dict(z=Z + 4)):
        a = valid(**kw, **TILED)
        assert lib.dl_cheb_round(ctypes.byref(a), None, 0, None) == INV, kw
        assert b"tiled operands must be 16-byte aligned" in lib.dl_last_error()
    # y overlapping x other than y == x with ldy == ldx
    for kw in (dict(mix_y=X + 64), dict(mix_y=X, mix_ldy=P + 4), dict(mix_y=X + BYTES - 4),
               dict(mix_y=X - BYTES + 4)):
        rc, msg, _ = call(valid(**kw))
        assert rc == INV and b"y overlaps x" in msg, (kw, msg)
    # ... and z other than y == z with ldy == ldz
    for kw in (dict(mix_y=Z + 64), dict(mix_y=Z, mix_ldy=P + 4), dict(mix_y=Z + BYTES - 4),
               dict(mix_y=Z - BYTES + 4), dict(mix_y=X, z=X + 4096), dict(mix_y=Z, ldz=P + 4)):
        rc, msg, _ = call(valid(**kw))
        assert rc == INV and b"y overlaps z" in msg, (kw, msg)
    rc, msg, _ = call(valid(mix_y=Z + 64 * 4 * N, **TILED))          # one tile into z
    assert rc == INV and b"y overlaps z" in msg
    assert call(valid(mix_y=Z + BYTES), plan_only=True)[0] == _lib.DL_OK   # adjacent: fine
    # plan pointer
    a = valid()
    assert lib.dl_cheb_round_plan(ctypes.byref(a), None) == INV
    assert b"plan is NULL" in lib.dl_last_error()
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
        assert rc == UNS and b"no halo rows, partition row sets or lagged deviation" in msg, \
            (kw, msg)
    # a plan path other than 1: the gather path (forced) ...
    monkeypatch.setenv("DLAMD_FORCE_GATHER", "1")
    rc, msg, _ = call(valid())
    assert rc == UNS and b"LDS tile kernel (plan path 1); this round plans path 2" in msg
    monkeypatch.delenv("DLAMD_FORCE_GATHER")
    # ... and the register-CSR paths: 4096 agents with per-edge weights (path 4), an irregular
    # graph of 3000 agents (path 5)
    big = dict(mix_ldx=1 << 16, mix_ldy=1 << 16, ldz=1 << 16, mix_n_params=1 << 16,
               mix_x=1 << 40, mix_y=1 << 42, z=1 << 44)
    rc, msg, _ = call(valid(mix_W=_lib.DlCsr(1 << 20, 1 << 21, 1 << 22, 4096, 5 * 4096, 5, 0, 0, 5),
                            **big))
    assert rc == UNS and b"this round plans path 4" in msg
    rc, msg, _ = call(valid(mix_W=_lib.DlCsr(1 << 20, 1 << 21, 1 << 22, 3000, 9000, 0, 1, 0, 3),
                            **big))
    assert rc == UNS and b"this round plans path 5" in msg
    # ... the forced register-CSR path in the column-tiled layout, y == z
    monkeypatch.setenv("DLAMD_FORCE_REG", "1")
    t = dict(mix_tile_cols=4, mix_ldx=0, mix_ldy=0, ldz=0, mix_n_params=64, mix_y=Z)
    rc, msg, _ = call(valid(mix_W=_lib.DlCsr(1 << 20, 1 << 21, 1 << 22, 1500, 7500, 5, 1, 1, 5),
                            **t))
    assert rc == UNS and b"this round plans path 4" in msg


def test_axpby_arguments():
    """dl_axpby's checks come before the launch; empty extents are a no-op."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    INV = _lib.DL_ERR_INVALID

    def axpby(s=X, lds=P, z=Z, ldz=P, out=Y, ldo=P, n=N, p=P):
        rc = lib.dl_axpby(s, lds, z, ldz, 1.5, -0.5, out, ldo, n, p, None)
        return rc, lib.dl_last_error()
    assert axpby(n=0)[0] == _lib.DL_OK and axpby(p=0)[0] == _lib.DL_OK
    for kw in (dict(s=None), dict(z=None), dict(out=None), dict(n=-1), dict(n=65536), dict(p=-1),
               dict(lds=P - 1), dict(ldz=P - 1), dict(ldo=P - 1)):
        rc, msg = axpby(**kw)
        assert rc == INV and b"dl_axpby: bad arguments" in msg, (kw, msg)
    for kw in (dict(out=X + 64), dict(out=X, ldo=P + 4), dict(out=X + BYTES - 4)):
        rc, msg = axpby(**kw)
        assert rc == INV and b"out must be s itself" in msg, (kw, msg)
    for kw in (dict(out=Z + 64), dict(out=Z, ldo=P + 4), dict(out=Z - BYTES + 4)):
        rc, msg = axpby(**kw)
        assert rc == INV and b"out must be z itself" in msg, (kw, msg)
