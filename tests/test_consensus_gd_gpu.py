"""BASELINE config c1 as one launch (dl_consensus_gd) against the synchronous restatement of the
reference's Titanic consensus GD (oracle/mixer_ref.consensus_gd, itself pinned bit for bit to the
reference's 4000-step asyncio run) and against that run's golden final weights.  The gradient's
dot products sum in a different order than numpy's BLAS, so the weights agree within 1e-9
relative; the Jacobi iteration counts exactly.

Below the Titanic runs: synthetic shapes through dl_consensus_gd itself against the numpy oracle
(tests/jacobi_oracle.py), and a tolerance-free tie of the kernel's Jacobi half to
dl_perron_round."""
import numpy as np
import pytest

from oracle import mixer_ref as M

pytestmark = pytest.mark.gpu


def titanic(golden):
    d = golden("titanic.npz")
    nt = int(d["n_test"])
    return d, d["X"][nt:], d["y"][nt:]


@pytest.mark.parametrize("topo_name,eps,iters", [("ring8", 10, 300), ("ring8", 1e-3, 60),
                                                 ("k4", 1e-6, 40), ("grid5", 1e-2, 50)])
def test_matches_synchronous_restatement(golden, cuda, topo_name, eps, iters):
    from distributed_learning_amd import workloads
    _, X, y = titanic(golden)
    topo = {"ring8": [(i, (i + 1) % 8) for i in range(8)],
            "k4": [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)],
            "grid5": [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4), (1, 3)]}[topo_name]
    want, ks = M.consensus_gd(topo, X, y, iters, conv_eps=eps)
    got, kd = workloads.consensus_gd_device(topo, X, y, iters, convergence_eps=eps, device=cuda)
    assert list(kd) == ks
    for t in want:
        np.testing.assert_allclose(got[t], want[t], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("eps,iters", [(10, 300), (1e-3, 60)])
def test_ring8_fast_averaging_weights(golden, cuda, eps, iters):
    """BASELINE c1's wording, "ring with fast-averaging weights": the ring's FDLA weights are one
    weight on every edge, w* = 1 / (3 - cos(2 pi / 8)) (find_optimal_weights, pinned by
    tests/test_fast_averaging.py), mixed as x' = x(1 - 2 w*) + w* sum_j x_j.  The one-launch run
    equals the restatement with that weight (same Jacobi counts, 1e-9 relative)."""
    from distributed_learning_amd import workloads
    from distributed_learning_amd.utils.fast_averaging import find_optimal_weights
    _, X, y = titanic(golden)
    topo = [(i, (i + 1) % 8) for i in range(8)]
    w, _ = find_optimal_weights(topo)
    assert np.allclose(w, w[0]) and abs(w[0] - 1 / (3 - np.cos(2 * np.pi / 8))) < 1e-8
    want, ks = M.consensus_gd(topo, X, y, iters, conv_eps=eps, edge_weight=float(w[0]))
    got, kd = workloads.consensus_gd_device(topo, X, y, iters, convergence_eps=eps, device=cuda,
                                            edge_weight=float(w[0]))
    assert list(kd) == ks
    for t in want:
        np.testing.assert_allclose(got[t], want[t], rtol=1e-9, atol=1e-12)


def test_reference_4000_step_run(golden, cuda):
    """The reference's ring-8, eps = 10, 4000-step asyncio run (golden final weights)."""
    from distributed_learning_amd import workloads
    d, X, y = titanic(golden)
    topo = [(i, (i + 1) % 8) for i in range(8)]
    got, kd = workloads.consensus_gd_device(topo, X, y, int(d["ring8_steps"]), convergence_eps=10,
                                            device=cuda)
    assert (kd == 1).all()
    w = np.stack([got[t] for t in d["ring8_tokens"].tolist()])
    np.testing.assert_allclose(w, d["ring8_eps10_final_w"], rtol=1e-9, atol=1e-12)
    acc = workloads.accuracy(w[0], d["X"][:int(d["n_test"])], d["y"][:int(d["n_test"])])
    assert abs(acc - 0.7978) < 6e-3   # the reference run's agent-0 accuracy


def test_validation(cuda):
    import ctypes

    from distributed_learning_amd import _lib
    lib = _lib.load()
    a = _lib.DlConsensusGdArgs()
    assert lib.dl_consensus_gd(ctypes.byref(a), 10, None) == _lib.DL_ERR_INVALID


# ---------------------------------------------------------------- synthetic shapes, direct ABI
# Titanic above reaches one shape of the kernel: 7 features, 4-8 agents, shards of ~90 rows held
# in LDS.  The cases of tests/jacobi_cases.GD_CASES (standard-normal X, labels +-1, non-zero start
# weights; conv_eps off every knife edge and the oracle's own error a tenth of the bound, both
# checked by tests/test_jacobi_oracle_cpu.py) reach the rest through dl_consensus_gd itself.
def _gd_args(cuda, c, **over):
    import torch

    from distributed_learning_amd import _lib
    t = dict(X=torch.from_numpy(c["X"]).to(cuda), y=torch.from_numpy(c["y"]).to(cuda),
             sp=torch.from_numpy(c["sp"]).to(cuda), rp=torch.from_numpy(c["rowptr"]).to(cuda),
             cl=torch.from_numpy(c["col"]).to(cuda), steps=torch.from_numpy(c["steps"]).to(cuda),
             w=torch.from_numpy(c["W0"].copy()).to(cuda),
             iters=torch.full((len(c["steps"]),), -1, dtype=torch.int32, device=cuda))
    sizes = np.diff(c["sp"])
    f = dict(n_agents=c["R"], n_features=c["F"], eps=c["eps"], conv_eps=c["conv_eps"],
             mean_weight=int(sizes.sum()) / len(sizes), tau=c["tau"], iterations=len(c["steps"]),
             max_iter=c["max_iter"])
    f.update(over)
    args = _lib.DlConsensusGdArgs(
        _lib.ptr(t["X"]), _lib.ptr(t["y"]), _lib.ptr(t["sp"]), f["n_agents"], f["n_features"],
        _lib.ptr(t["rp"]), _lib.ptr(t["cl"]), f["eps"], f["conv_eps"], f["mean_weight"],
        f["tau"], _lib.ptr(t["steps"]), f["iterations"], f["max_iter"], _lib.ptr(t["w"]),
        _lib.ptr(t["iters"]))
    return args, t


def _gd_run(cuda, c, **over):
    import ctypes

    from distributed_learning_amd import _lib
    args, t = _gd_args(cuda, c, **over)
    rc = _lib.load().dl_consensus_gd(ctypes.byref(args), int(c["sp"][-1]),
                                     _lib.stream_handle(cuda))
    return rc, t["w"].cpu().numpy(), t["iters"].cpu().tolist()


def test_zero_steps_equal_perron_rounds(cuda):
    """Tolerance-free: with every step size 0 the local step leaves the (non-zero, finite)
    weights as they are (w - 0 * g == w), so T = 3 iterations are T successive fp64
    dl_perron_round calls weighted by the shard sizes -- the same pre-scale (w * n) / mean and
    the same Jacobi arithmetic -- bit for bit, with the same iteration counts.  12 agents (a
    second pass of the 8 waves), shards of 1, 2, 63, 64, 65, ... rows, a start from non-zero
    weights in every iteration."""
    import torch

    import jacobi_cases as C
    import jacobi_oracle as O
    from distributed_learning_amd import engine
    c = C.gd_case("crosscheck")
    assert not c["steps"].any() and len(c["steps"]) == 3
    rc, W, ks = _gd_run(cuda, c)
    assert rc == 0
    sizes = np.diff(c["sp"]).astype(np.float64)
    Y = torch.from_numpy(c["W0"].copy()).to(cuda)
    rp, cl = torch.from_numpy(c["rowptr"]).to(cuda), torch.from_numpy(c["col"]).to(cuda)
    ks_perron = [engine.perron_round(Y, rp, cl, c["eps"], c["conv_eps"],
                                     weight=torch.from_numpy(sizes).to(cuda),
                                     mean_weight=float(sizes.sum()) / len(sizes),
                                     max_iter=c["max_iter"]) for _ in c["steps"]]
    assert ks == ks_perron == C.gd_want("crosscheck")[1]
    assert O.same_bits(W, Y.cpu().numpy())
    assert O.same_bits(W, C.gd_want("crosscheck")[0])     # and both are the oracle's bits


@pytest.mark.parametrize("name", ["a_ring12_f16", "b_torus20_f1", "c_global_f16", "d_isolated",
                                  "e_cut2"])
def test_synthetic_shapes_match_oracle(cuda, name):
    """10 iterations with real steps against logreg_step + jacobi_round:
    a  12 agents (more than the 8 waves), 16 features (the j == lane select at its limit),
       shards of 1, 2, 63, 64, 65, ... rows (one row, shorter than a wave, a wave, past it);
    b  20 agents on a 4 x 5 torus, one feature;
    c  1400 rows x 16 features: rows * (F + 1) * 8 exceeds LDS, the shards are read from global
       memory (x_in_lds == 0);
    d  an agent without neighbours;
    e  max_iter = 2 with conv_eps = 0: every round cut at 2.
    The weights agree within the bound this kernel's summation order was given above; the Jacobi
    iteration counts exactly."""
    import jacobi_cases as C
    c = C.gd_case(name)
    want, ks_want, _ = C.gd_want(name)
    rc, W, ks = _gd_run(cuda, c)
    assert rc == 0
    print(f"{name}: max rel err {np.max(np.abs(W - want) / np.abs(want)):.3e}, "
          f"max abs err {np.max(np.abs(W - want)):.3e}, iterations {ks}")
    assert ks == ks_want
    np.testing.assert_allclose(W, want, rtol=1e-9, atol=1e-12)


def test_refusals(cuda):
    import jacobi_cases as C
    from distributed_learning_amd import _lib
    c = C.gd_case("a_ring12_f16")
    for over, status in ((dict(n_features=17), _lib.DL_ERR_INVALID),
                         (dict(mean_weight=0.0), _lib.DL_ERR_INVALID),
                         # 3 * 512 * 16 * 8 B of weights and ping-pong alone exceed LDS
                         (dict(n_agents=512), _lib.DL_ERR_UNSUPPORTED)):
        rc, W, ks = _gd_run(cuda, c, **over)
        assert rc == status, over
        assert np.array_equal(W, c["W0"]) and ks == [-1] * len(c["steps"]), over
