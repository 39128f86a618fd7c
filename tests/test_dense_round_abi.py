"""CPU checks of dl_dense_round's C ABI: the struct layout, the symbols, every refusal with its
status and a text naming the value before any device call, and the plan of the GPU test's shapes
(runs without a GPU)."""
import ctypes
import os
import subprocess

import pytest

# dummy device addresses, never dereferenced: 64 agents x 4096 params, far apart
X, Y, G, W = 1 << 30, 1 << 32, 1 << 36, 1 << 38
N, P = 64, 4096
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def valid(**kw):
    from distributed_learning_amd import _lib
    a = _lib.DlDenseRoundArgs(X, P, Y, P, None, 0, 0.0, W, N, N, P, 0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_the_struct_layout_agrees_with_c(tmp_path):
    from distributed_learning_amd import _lib
    fields = [f for f, _ in _lib.DlDenseRoundArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dlamd.h"\nint main(void) {\n'
                   + "".join(f'printf("%zu ", offsetof(dl_dense_round_args, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(dl_dense_round_args)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    want = [getattr(_lib.DlDenseRoundArgs, f).offset for f in fields]
    assert got == want + [ctypes.sizeof(_lib.DlDenseRoundArgs)]


@pytest.mark.parametrize("mutation,text", [
    (None, b"args is NULL"),
    (dict(x=None), b"null x/y/w"),
    (dict(w=None), b"null x/y/w"),
    (dict(n_rows=1), b"n_rows must be in 2..256 (got 1)"),
    (dict(n_rows=257, ldw=257), b"n_rows must be in 2..256 (got 257)"),
    (dict(ldx=P - 1), b"ldx 4095 < n_params 4096"),
    (dict(g=G, ldg=P - 4), b"ldg 4092 < n_params 4096"),
    (dict(ldw=N - 1), b"ldw 63 < n_rows 64"),
    (dict(tile_cols=24, ldx=0, ldy=0), b"multiple of 16 up to 128 (got 24)"),
    (dict(tile_cols=144, ldx=0, ldy=0), b"multiple of 16 up to 128 (got 144)"),
    (dict(tile_cols=64, ldx=0, ldy=N - 1), b"tiled ld: ldy 63"),
    (dict(y=X + 64), b"y overlaps x"),
    (dict(g=G, ldg=P, y=G + 4 * P * (N - 1)), b"y overlaps g"),
    (dict(y=W - 4 * P * N + 16), b"y overlaps w"),
])
def test_plan_and_round_refuse_alike(mutation, text):
    from distributed_learning_amd import _lib
    lib = _lib.load()
    ref = ctypes.byref(valid(**mutation)) if mutation is not None else None
    rc, msg = lib.dl_dense_round_plan(ref, ctypes.byref(_lib.DlMixPlan())), lib.dl_last_error()
    assert rc == _lib.DL_ERR_INVALID and text in msg, (rc, msg)
    assert lib.dl_dense_round(ref, None) == rc and lib.dl_last_error() == msg


@pytest.mark.parametrize("n,p", [(2, 7), (33, 129), (64, 4096), (100, 777), (129, 3 * 128 + 5),
                                 (256, 777)])
def test_the_plan_of_an_accepted_round(n, p):
    from distributed_learning_amd import _lib
    lib, pl = _lib.load(), _lib.DlMixPlan()
    a = valid(n_rows=n, ldw=n, n_params=p, ldx=p + 3, ldy=p + 3)
    assert lib.dl_dense_round_plan(ctypes.byref(a), ctypes.byref(pl)) == _lib.DL_OK, \
        lib.dl_last_error()
    assert lib.dl_dense_round_plan(ctypes.byref(a), None) == _lib.DL_ERR_INVALID
    assert b"plan is NULL" in lib.dl_last_error()
    assert pl.path == 6 and pl.lds_bytes <= 163840 and pl.grid >= 1
    assert pl.n_tiles == -(-p // pl.tile_cols)
    assert lib.dl_abi_version() == 10
    assert {"dl_dense_round", "dl_dense_round_plan"} <= set(_lib.SIGNATURES)
