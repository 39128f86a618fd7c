"""CPU checks of dl_trim_round's C ABI: every refusal comes back with its status and its own text
before any device call; an accepted round plans what dl_mix_round plans (runs without a GPU)."""
import ctypes

import pytest

# dummy device addresses, never dereferenced: 64 agents x 4096 params, far apart
X, Y, G = 1 << 30, 1 << 32, 1 << 36
N, P = 64, 4096
BIG = dict(mix_ldx=1 << 16, mix_ldy=1 << 16, mix_n_params=1 << 16, mix_x=1 << 40, mix_y=1 << 42)


def valid(**kw):
    """A 4-regular graph, trim 1; mix_* set dl_mix_args fields, mix_W the CSR's sizes and flags."""
    from distributed_learning_amd import _lib
    a = _lib.DlTrimRoundArgs()
    a.mix.x, a.mix.y, a.mix.ldx, a.mix.ldy, a.mix.n_params = X, Y, P, P, P
    a.trim, a.max_row_nnz, a.min_row_nnz = 1, 5, 5
    kw.setdefault("mix_W", (N, 5 * N, 5, 1, 1, 5))
    for k, v in kw.items():
        if k == "mix_W":
            v = _lib.DlCsr(1 << 20, 1 << 21, 1 << 22, *v)
        setattr(a.mix if k.startswith("mix_") else a, k[4:] if k.startswith("mix_") else k, v)
    return a


@pytest.mark.parametrize("mutation,env,status,text", [
    (None, None, "INVALID", b"args is NULL"),
    (dict(mix_x=None), None, "INVALID", b"null x/y"),
    (dict(trim=-1), None, "INVALID", b"trim must be in 0..7"),
    (dict(max_row_nnz=1, min_row_nnz=1, trim=0), None, "INVALID", b"max_row_nnz must be in 2..17"),
    (dict(max_row_nnz=4, min_row_nnz=5), None, "INVALID", b"below min_row_nnz"),
    (dict(min_row_nnz=3), None, "INVALID", b"trim 1 needs min_row_nnz >= 4"),
    (dict(trim=0, min_row_nnz=0), None, "INVALID", b"trim 0 needs min_row_nnz >= 1"),
    (dict(max_row_nnz=4, min_row_nnz=4), None, "INVALID", b"contradicts the promised row lengths"),
    (dict(mix_y=X + 64), None, "INVALID", b"y overlaps x"),
    (dict(mix_g=G, mix_ldg=P - 1), None, "INVALID", b"ldg < n_params"),
    (dict(mix_halo=1 << 38, mix_n_halo=4, mix_ldh=P), None, "UNSUPPORTED", b"no halo rows"),
    (dict(mix_n_local_src=N + 8), None, "UNSUPPORTED", b"partition row sets"),
    (dict(mix_mean_prev=1 << 38), None, "UNSUPPORTED", b"lagged deviation"),
    ({}, "DLAMD_FORCE_GATHER", "UNSUPPORTED", b"this round plans path 2"),
    (dict(mix_W=(4096, 5 * 4096, 5, 0, 0, 5), **BIG), None, "UNSUPPORTED",
     b"this round plans path 4"),
    (dict(mix_W=(3000, 15000, 0, 1, 0, 4), max_row_nnz=9, min_row_nnz=4, **BIG), None,
     "UNSUPPORTED", b"this round plans path 5"),
])
def test_plan_and_round_refuse_alike(monkeypatch, mutation, env, status, text):
    from distributed_learning_amd import _lib
    lib = _lib.load()
    if env:
        monkeypatch.setenv(env, "1")
    a = valid(**mutation) if mutation is not None else None
    ref = ctypes.byref(a) if a is not None else None
    rc, msg = lib.dl_trim_round_plan(ref, ctypes.byref(_lib.DlMixPlan())), lib.dl_last_error()
    assert rc == getattr(_lib, "DL_ERR_" + status) and text in msg, (rc, msg)
    assert lib.dl_trim_round(ref, None, 0, None) == rc and lib.dl_last_error() == msg


@pytest.mark.parametrize("kw", [
    dict(),                                                          # regular, 4 neighbours
    dict(mix_y=X, mix_g=G, mix_ldg=P, mix_dev_sq=1 << 38, trim=0),   # in place, g, deviation
    dict(mix_tile_cols=64, mix_ldx=0, mix_ldy=0, mix_n_params=4100,  # column-tiled, irregular
         mix_W=(300, 2500, 0, 0, 0, 8), trim=3, max_row_nnz=9, min_row_nnz=8)])
def test_an_accepted_round_plans_what_dl_mix_round_plans(kw):
    from distributed_learning_amd import _lib
    lib, a, pl, pm = _lib.load(), valid(**kw), _lib.DlMixPlan(), _lib.DlMixPlan()
    assert lib.dl_trim_round_plan(ctypes.byref(a), ctypes.byref(pl)) == _lib.DL_OK, \
        lib.dl_last_error()
    assert lib.dl_trim_round_plan(ctypes.byref(a), None) == _lib.DL_ERR_INVALID
    assert b"plan is NULL" in lib.dl_last_error()
    if a.mix.dev_sq:   # a deviation without a workspace: dl_mix_round's refusal
        for ws in ((None, 0), (1 << 40, 16)):
            assert lib.dl_trim_round(ctypes.byref(a), *ws, None) == _lib.DL_ERR_WORKSPACE
            assert b"workspace" in lib.dl_last_error()
    a.mix.y = Y   # (the plain round refuses y == x; the plan does not depend on it)
    assert lib.dl_mix_plan_query(ctypes.byref(a.mix), ctypes.byref(pm)) == _lib.DL_OK
    assert pl.path == 1 and lib.dl_abi_version() == 10 and "dl_trim_round" in _lib.SIGNATURES
    for f in ("path", "tile_cols", "grid", "n_tiles"):
        assert getattr(pl, f) == getattr(pm, f), f
