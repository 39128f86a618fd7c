"""CPU checks of dl_edge_sqdist's and dl_clip_weights' C ABI: every refusal comes back with its
status and its own text before any device call; an accepted pass plans what dl_mix_round plans
(runs without a GPU)."""
import ctypes

import pytest

# dummy device addresses, never dereferenced: 64 agents x 4096 params, far apart
X, G, E = 1 << 30, 1 << 36, 1 << 38
N, P = 64, 4096
BIG = dict(mix_ldx=1 << 16, mix_n_params=1 << 16, mix_x=1 << 40)


def valid(**kw):
    """A 4-regular graph; mix_* set dl_mix_args fields, mix_W the CSR's sizes and flags."""
    from distributed_learning_amd import _lib
    a = _lib.DlEdgeSqdistArgs()
    a.mix.x, a.mix.ldx, a.mix.n_params = X, P, P
    a.edge_sq, a.max_row_nnz, a.min_row_nnz = E, 5, 5
    kw.setdefault("mix_W", (N, 5 * N, 5, 1, 1, 5))
    for k, v in kw.items():
        if k == "mix_W":
            v = _lib.DlCsr(1 << 20, 1 << 21, 1 << 22, *v)
        setattr(a.mix if k.startswith("mix_") else a, k[4:] if k.startswith("mix_") else k, v)
    return a


@pytest.mark.parametrize("mutation,env,status,text", [
    (None, None, "INVALID", b"args is NULL"),
    (dict(edge_sq=None), None, "INVALID", b"null x/edge_sq"),
    (dict(mix_y=1 << 32, mix_ldy=P), None, "INVALID", b"y, dev_sq, dev_max and mean must be NULL"),
    (dict(mix_dev_sq=1 << 32), None, "INVALID", b"y, dev_sq, dev_max and mean must be NULL"),
    (dict(max_row_nnz=18), None, "INVALID", b"max_row_nnz must be in 2..17"),
    (dict(max_row_nnz=1, min_row_nnz=1), None, "INVALID", b"max_row_nnz must be in 2..17"),
    (dict(max_row_nnz=4, min_row_nnz=5), None, "INVALID", b"below min_row_nnz"),
    (dict(max_row_nnz=4, min_row_nnz=4), None, "INVALID", b"contradicts the promised row lengths"),
    (dict(edge_sq=X + 64), None, "INVALID", b"edge_sq overlaps x or g"),
    (dict(mix_g=G, mix_ldg=P - 1), None, "INVALID", b"ldg < n_params"),
    (dict(mix_n_local_src=N + 8), None, "UNSUPPORTED", b"partition row sets"),
    ({}, "DLAMD_FORCE_GATHER", "UNSUPPORTED", b"this round plans path 2"),
    (dict(mix_W=(4096, 5 * 4096, 5, 0, 0, 5), **BIG), None, "UNSUPPORTED",
     b"this round plans path 4"),
    # 1100 agents at 16 columns a tile are 8 rows a thread; 16 slots of them are 128 accumulators
    (dict(mix_W=(1100, 11000, 10, 0, 0, 10), max_row_nnz=10, min_row_nnz=10, mix_tile_cols=16,
          mix_ldx=0), None, "UNSUPPORTED", b"accumulator registers.*smaller tile_cols"),
])
def test_plan_and_pass_refuse_alike(monkeypatch, mutation, env, status, text):
    import re
    from distributed_learning_amd import _lib
    lib = _lib.load()
    if env:
        monkeypatch.setenv(env, "1")
    a = valid(**mutation) if mutation is not None else None
    ref = ctypes.byref(a) if a is not None else None
    rc, msg = lib.dl_edge_sqdist_plan(ref, ctypes.byref(_lib.DlMixPlan())), lib.dl_last_error()
    assert rc == getattr(_lib, "DL_ERR_" + status) and re.search(text, msg), (rc, msg)
    assert lib.dl_edge_sqdist(ref, None, 0, None) == rc and lib.dl_last_error() == msg


@pytest.mark.parametrize("kw", [
    dict(),                                                          # regular, 4 neighbours
    dict(mix_g=G, mix_ldg=P),
    dict(mix_tile_cols=64, mix_ldx=0, mix_n_params=4100,             # column-tiled, irregular
         mix_W=(300, 2500, 0, 0, 0, 8), max_row_nnz=9, min_row_nnz=8)])
def test_an_accepted_pass_plans_what_dl_mix_round_plans_and_needs_its_workspace(kw):
    from distributed_learning_amd import _lib
    lib, a, pl, pm = _lib.load(), valid(**kw), _lib.DlMixPlan(), _lib.DlMixPlan()
    assert lib.dl_edge_sqdist_plan(ctypes.byref(a), ctypes.byref(pl)) == _lib.DL_OK, \
        lib.dl_last_error()
    assert lib.dl_edge_sqdist_plan(ctypes.byref(a), None) == _lib.DL_ERR_INVALID
    assert b"plan is NULL" in lib.dl_last_error()
    need = lib.dl_edge_sqdist_workspace_bytes(a.mix.W.n_rows, a.max_row_nnz, a.mix.n_params)
    assert need >= pl.grid * a.mix.W.n_rows * (a.max_row_nnz - 1) * 4
    for ws in ((None, 0), (None, need), (1 << 42, 16), ((1 << 42) + 4, need)):
        assert lib.dl_edge_sqdist(ctypes.byref(a), *ws, None) == _lib.DL_ERR_WORKSPACE, ws
        assert b"workspace" in lib.dl_last_error()
    a.mix.y, a.mix.ldy = 1 << 32, a.mix.ldx
    assert lib.dl_mix_plan_query(ctypes.byref(a.mix), ctypes.byref(pm)) == _lib.DL_OK
    assert pl.path == 1 and lib.dl_abi_version() == 10
    assert {"dl_edge_sqdist", "dl_edge_sqdist_plan", "dl_edge_sqdist_workspace_bytes",
            "dl_clip_weights"} <= set(_lib.SIGNATURES)
    for f in ("path", "tile_cols", "grid", "n_tiles"):
        assert getattr(pl, f) == getattr(pm, f), f


@pytest.mark.parametrize("kw,text", [
    (None, b"args is NULL"),
    (dict(edge_sq=None), b"null row_ptr/col/w/edge_sq/w_out"),
    (dict(w_out=None), b"null row_ptr/col/w/edge_sq/w_out"),
    (dict(tau=None, drop=0), b"drop must be in 1..16"),
    (dict(max_row_nnz=18), b"max_row_nnz must be in 2..17")])
def test_clip_weights_refusals(kw, text):
    from distributed_learning_amd import _lib
    lib, a = _lib.load(), None
    if kw is not None:
        a = _lib.DlClipWeightsArgs(_lib.DlCsr(1 << 20, 1 << 21, 1 << 22, N, 5 * N, 5, 1, 1, 5),
                                   E, 1 << 39, 0, 5, 1 << 40, None)
        for k, v in kw.items():
            setattr(a, k, v)
    rc = lib.dl_clip_weights(ctypes.byref(a) if a is not None else None, None)
    assert rc == _lib.DL_ERR_INVALID and text in lib.dl_last_error(), lib.dl_last_error()
