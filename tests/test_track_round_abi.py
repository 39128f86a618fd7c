"""CPU checks of the gradient-tracking round's C ABI (dl_track_round, dl_track_round_plan): the
struct layout agrees between C and ctypes, and every refusal the header states comes back with
its status and message before any device call (runs without a GPU)."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("d", "ldd", "d_out", "lddo", "g_old", "ldq")


def test_struct_layout_matches_c(tmp_path):
    from distributed_learning_amd import _lib
    prog = tmp_path / "layout.c"
    offs = ",".join(f"offsetof(dl_track_round_args, {f})" for f in FIELDS)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dlamd.h"\n'
                    'int main(void){printf("' + "%zu " * (len(FIELDS) + 1) + '\\n",'
                    'sizeof(dl_track_round_args),' + offs + ');return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                        check=True).stdout.split()]
    A = _lib.DlTrackRoundArgs
    assert c == [ctypes.sizeof(A)] + [getattr(A, f).offset for f in FIELDS]
    assert A.mix.offset == 0 and A.d.offset == ctypes.sizeof(_lib.DlMixArgs)


def test_symbols_are_additive():
    """New symbols, the ABI version unchanged: callers detect the round by the symbol."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    for name in ("dl_track_round", "dl_track_round_plan"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.dl_abi_version() == 10 and _lib.ABI_VERSION == 10


# dummy device addresses, never dereferenced: 64 agents x 4096 params, far apart
X, Y, G, D, DO, Q = 1 << 30, 1 << 32, 1 << 34, 1 << 36, 1 << 37, 1 << 38
N, P = 64, 4096
BYTES = N * P * 4
TILED = dict(mix_tile_cols=64, mix_ldx=0, mix_ldy=0, mix_ldg=0, ldd=0, lddo=0, ldq=0)


def valid(**kw):
    from distributed_learning_amd import _lib
    a = _lib.DlTrackRoundArgs()
    m = a.mix
    m.x, m.y, m.g = X, Y, G
    m.ldx = m.ldy = m.ldg = P
    m.n_params = P
    m.lr = 0.1
    m.W = _lib.DlCsr(1 << 20, 1 << 21, 1 << 22, N, 5 * N, 5, 1, 1, 5)
    a.d, a.d_out, a.g_old = D, DO, Q
    a.ldd = a.lddo = a.ldq = P
    for k, v in kw.items():
        if k.startswith("mix_"):
            setattr(a.mix, k[4:], v)
        else:
            setattr(a, k, v)
    return a


def call(a, plan_only=False):
    """(status, message, plan) of dl_track_round_plan and, unless plan_only, of dl_track_round
    too (they must agree)."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    pl = _lib.DlMixPlan()
    ref = ctypes.byref(a) if a is not None else None
    rc = lib.dl_track_round_plan(ref, ctypes.byref(pl))
    msg = lib.dl_last_error()
    if not plan_only:
        rc2 = lib.dl_track_round(ref, None, 0, None)
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
    # x' = x and d' = d are accepted, row-major and column-tiled
    for kw in (dict(mix_y=X), dict(d_out=D), dict(mix_y=X, d_out=D)):
        assert call(valid(**kw), plan_only=True)[0] == _lib.DL_OK, kw
        assert call(valid(**kw, **TILED), plan_only=True)[0] == _lib.DL_OK, kw
    # padded rows: every stride its own
    assert call(valid(mix_ldx=P + 4, mix_ldy=P + 8, mix_ldg=P + 12, ldd=P + 16, lddo=P + 20,
                      ldq=P + 24), plan_only=True)[0] == _lib.DL_OK
    # a deviation without a workspace is the round's DL_ERR_WORKSPACE, as dl_mix_round's; the plan
    # query has no workspace to refuse
    a = valid(mix_dev_sq=1 << 40, mix_dev_max=1 << 41)
    lib = _lib.load()
    assert lib.dl_track_round_plan(ctypes.byref(a), ctypes.byref(pl)) == _lib.DL_OK
    assert lib.dl_track_round(ctypes.byref(a), None, 0, None) == _lib.DL_ERR_WORKSPACE
    assert b"workspace" in lib.dl_last_error()
    assert lib.dl_track_round(ctypes.byref(a), 1 << 42, 16, None) == _lib.DL_ERR_WORKSPACE
    assert b"workspace" in lib.dl_last_error()


def test_invalid_arguments():
    from distributed_learning_amd import _lib
    lib = _lib.load()
    INV = _lib.DL_ERR_INVALID
    rc, msg, _ = call(None)
    assert rc == INV and b"args is NULL" in msg
    for f in ("mix_x", "mix_y", "mix_g", "d", "d_out", "g_old"):
        rc, msg, _ = call(valid(**{f: None}))
        assert rc == INV and b"null x/y/d/d_out/g/g_old" in msg, (f, msg)
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
    # a tracker or gradient not laid out as x
    for f in ("ldd", "lddo", "ldq"):
        rc, msg, _ = call(valid(**{f: P - 1}))
        assert rc == INV and b"d, d_out and g_old laid out as x" in msg, (f, msg)
        for v in (N - 1, -1):                                      # tiled: block rows < n_rows
            rc, msg, _ = call(valid(**{**TILED, f: v}))
            assert rc == INV and b"d, d_out and g_old laid out as x" in msg, (f, v, msg)
    # alignment the round refuses: column-tiled operands off 16 bytes, from the round itself --
    # the plan query stops before
    for kw in (dict(mix_x=X + 4), dict(mix_g=G + 4), dict(d=D + 4), dict(d_out=DO + 4),
               dict(g_old=Q + 4)):
        a = valid(**kw, **TILED)
        assert lib.dl_track_round(ctypes.byref(a), None, 0, None) == INV, kw
        assert b"tiled operands must be 16-byte aligned" in lib.dl_last_error()
    # d_out overlapping x, y, g or g_old in any way
    for name, base in (("x", X), ("y", Y), ("g", G), ("g_old", Q)):
        for off in (0, 64, BYTES - 4, -BYTES + 4):
            rc, msg, _ = call(valid(d_out=base + off))
            assert rc == INV and b"dl_track_round: d_out overlaps " + name.encode() in msg, \
                (name, off, msg)
    # ... and d other than d_out == d with lddo == ldd
    for kw in (dict(d_out=D + 64), dict(d_out=D, lddo=P + 4), dict(d_out=D + BYTES - 4),
               dict(d_out=D - BYTES + 4)):
        rc, msg, _ = call(valid(**kw))
        assert rc == INV and b"d_out overlaps d (d_out may be d itself" in msg, (kw, msg)
    rc, msg, _ = call(valid(d_out=D + 64 * 4 * N, **TILED))           # one tile into d
    assert rc == INV and b"d_out overlaps d" in msg
    # y overlapping d or g_old (the tracking round's texts), g (the plain round's) ...
    for name, base in (("d", D), ("g_old", Q)):
        for off in (0, 64, BYTES - 4, -BYTES + 4):
            rc, msg, _ = call(valid(mix_y=base + off))
            assert rc == INV and b"dl_track_round: y overlaps " + name.encode() in msg, \
                (name, off, msg)
    rc, msg, _ = call(valid(mix_y=D, d_out=D))                         # y on the in-place tracker
    assert rc == INV and b"overlaps" in msg
    for off in (0, 64, BYTES - 4):
        rc, msg, _ = call(valid(mix_y=G + off))
        assert rc == INV and b"y overlaps g" in msg
    # ... and x other than y == x with ldy == ldx
    for kw in (dict(mix_y=X + 64), dict(mix_y=X, mix_ldy=P + 4), dict(mix_y=X + BYTES - 4),
               dict(mix_y=X - BYTES + 4)):
        rc, msg, _ = call(valid(**kw))
        assert rc == INV and b"y overlaps x" in msg, (kw, msg)
    assert call(valid(d_out=D + BYTES, mix_y=X + BYTES), plan_only=True)[0] == _lib.DL_OK  # adjacent
    # plan pointer
    a = valid()
    assert lib.dl_track_round_plan(ctypes.byref(a), None) == INV
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
        assert rc == UNS and b"no halo rows, partition row sets or lagged deviation" in msg, \
            (kw, msg)
    # a plan path other than 1: the gather path (forced) ...
    monkeypatch.setenv("DLAMD_FORCE_GATHER", "1")
    rc, msg, _ = call(valid())
    assert rc == UNS and b"LDS tile kernel (plan path 1); this round plans path 2" in msg
    monkeypatch.delenv("DLAMD_FORCE_GATHER")
    # ... and the register-CSR paths: 4096 agents with per-edge weights (path 4), an irregular
    # graph of 3000 agents (path 5)
    ld = 1 << 16
    big = dict(mix_ldx=ld, mix_ldy=ld, mix_ldg=ld, ldd=ld, lddo=ld, ldq=ld, mix_n_params=ld,
               mix_x=1 << 40, mix_y=1 << 42, mix_g=1 << 44, d=1 << 46, d_out=1 << 48,
               g_old=1 << 50)
    rc, msg, _ = call(valid(mix_W=_lib.DlCsr(1 << 20, 1 << 21, 1 << 22, 4096, 5 * 4096, 5, 0, 0, 5),
                            **big))
    assert rc == UNS and b"this round plans path 4" in msg
    rc, msg, _ = call(valid(mix_W=_lib.DlCsr(1 << 20, 1 << 21, 1 << 22, 3000, 9000, 0, 1, 0, 3),
                            **big))
    assert rc == UNS and b"this round plans path 5" in msg
    # ... the forced register-CSR path in the column-tiled layout, in place
    monkeypatch.setenv("DLAMD_FORCE_REG", "1")
    t = dict(TILED, mix_tile_cols=4, mix_n_params=64, mix_y=X, d_out=D)
    rc, msg, _ = call(valid(mix_W=_lib.DlCsr(1 << 20, 1 << 21, 1 << 22, 1500, 7500, 5, 1, 1, 5),
                            **t))
    assert rc == UNS and b"this round plans path 4" in msg
