"""``dl_perron_round`` (engine.perron_round) against the plain-numpy oracle
(tests/jacobi_oracle.py), bit for bit in fp64 and in fp32, values and iteration count, at the
shapes where its two kernels and the host loop between them change path (tests/jacobi_cases.py;
tests/test_jacobi_oracle_cpu.py holds every case's convergence tests 1e-6 relative away from
their conv_eps, so a failure here is never a knife-edge input):

single launch (perron_single_kernel): weights on / off, per-agent conv_eps with one strict agent
deciding the count, a slice of a wider tensor (ldy > n_params, padding untouched), an agent
without neighbours, a loop cut by max_iter = 1, 2, 3, the widest single-launch width;
host-iterated tiles (perron_step_kernel): one column past that width (the tile wider than the
matrix), three tiles with a ragged last one, the pre-scale that applies in iteration 1 only, odd
and even iteration counts (the result ends in the workspace or in y), per-agent conv_eps, the
row limit where a tile is one column wide, and the refusal one row above it;
both: -0.0 neighbourhoods (np.sum folds from +0.0), NaN and infinities.

With -ffp-contract=off every operation of the kernels is one numpy operation of the oracle, so
nothing here has a tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import jacobi_cases as C
import jacobi_oracle as O

pytestmark = pytest.mark.gpu

PAD_VALUE = -7.2519531e+11      # what the columns [n_params, ldy) hold before and after


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)


def _round(c, cuda):
    """Run one case: returns (values [n, P], padding [n, pad], k)."""
    from distributed_learning_amd import engine
    n, P, pad = c["n"], c["P"], c["pad"]
    big = np.full((n, P + pad), PAD_VALUE, c["dtype"])
    big[:, :P] = c["Y0"]
    B = torch.from_numpy(big).to(cuda)
    weight = None if c["weight"] is None else torch.tensor(c["weight"], dtype=torch.float64,
                                                           device=cuda)
    rows = None if c["conv_rows"] is None else torch.tensor(c["conv_rows"], dtype=torch.float64,
                                                            device=cuda)
    k = engine.perron_round(B[:, :P], _i32(c["rowptr"], cuda), _i32(c["col"], cuda), c["eps"],
                            c["conv_eps"], weight=weight, mean_weight=c["mean_w"],
                            max_iter=c["max_iter"], conv_eps_rows=rows)
    out = B.cpu().numpy()
    return out[:, :P], out[:, P:], k


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", list(C.PERRON_CASES))
def test_perron_round_equals_oracle(cuda, name, dt):
    c = C.perron_case(name, dt)
    want, k_want = c["want"]
    tp = C.perron_tile_cols(c["dtype"], c["n"], c["P"])
    assert (tp == c["P"]) == (C.PERRON_CASES[name]["P"] in (33, "limit")), "planner path moved"
    got, padding, k = _round(c, cuda)
    assert k == k_want
    if np.isnan(want).any():
        assert np.array_equal(got, want, equal_nan=True)
    assert O.same_bits(got, want), (
        f"{int((got != want).sum())} values differ, max abs {np.nanmax(np.abs(got - want)):.3e}; "
        f"signs differ at {np.argwhere(np.signbit(got) != np.signbit(want))[:4].tolist()}")
    assert padding.shape[1] == c["pad"]
    assert O.same_bits(padding, np.full_like(padding, PAD_VALUE))


def test_row_limit_one_column_tiles(cuda):
    """20478 fp64 agents: one column of the matrix fills the LDS tile (TP == 1), so P = 3 runs
    as three workgroups; max_iter = 2 ends in y without a copy-back."""
    from distributed_learning_amd import engine
    c = C.row_limit_case()
    Y = torch.from_numpy(c["Y0"]).to(cuda)
    k = engine.perron_round(Y, _i32(c["rowptr"], cuda), _i32(c["col"], cuda), c["eps"], 0.0,
                            max_iter=2)
    assert k == 2 == c["want"][1]
    assert O.same_bits(Y.cpu().numpy(), c["want"][0])


def test_above_row_limit_is_refused(cuda):
    """One agent more and not even one column fits: DL_ERR_UNSUPPORTED, nothing launched (y and
    iters_out keep their bits)."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    n = C.ROW_LIMIT + 1
    rowptr, col = O.ring_csr(n)
    Y0 = np.random.default_rng(5).standard_normal((n, 3))
    Y = torch.from_numpy(Y0).to(cuda)
    rp, cl = _i32(rowptr, cuda), _i32(col, cuda)
    iters = torch.full((1,), -5, dtype=torch.int32, device=cuda)
    ws = torch.empty(lib.dl_perron_workspace_bytes(1, n, 3), dtype=torch.uint8, device=cuda)
    args = _lib.DlPerronArgs(1, _lib.ptr(Y), 3, n, 3, _lib.ptr(rp), _lib.ptr(cl), None, 1.0,
                             O.max_degree_eps(rowptr), 0.0, 2, _lib.ptr(iters), None)
    rc = lib.dl_perron_round(ctypes.byref(args), _lib.ptr(ws), ws.numel(),
                             _lib.stream_handle(cuda))
    assert rc == _lib.DL_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert int(iters.item()) == -5 and O.same_bits(Y.cpu().numpy(), Y0)
