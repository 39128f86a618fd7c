"""GPU parity of the dense round (dl_dense_round) with its rule (include/dlamd.h): the k-ordered
fp32 fma chain of oracle.cref.bgemm applied to the numpy local step, bit for bit."""
import functools

import numpy as np
import pytest
import torch

from oracle import cref
from test_mix_gpu import check_dev
from test_sgd_round_gpu import dev_t, regular_csr, same

pytestmark = pytest.mark.gpu
ROUNDS, LR = 3, 0.05
SHAPES = [(2, 7), (33, 129), (64, 4096), (100, 777), (129, 3 * 128 + 5), (256, 777)]


def E():
    from distributed_learning_amd import engine
    return engine


def rule(Wd, X, G=None, lr=0.0):
    """One round of the rule: cref.bgemm of Wd and the fp32 local step, held to (N + 1) 2^-24
    (|Wd| |S|) of the fp64 product -- N roundings of the chain and one of margin."""
    S = np.ascontiguousarray(X if G is None else X - np.float32(lr) * G)
    (n, P), Y = S.shape, np.empty_like(S)
    cref.bgemm(1, n, P, n, np.ascontiguousarray(Wd), n, 0, 0, S, P, 0, 0, Y, P, 0)
    W64, S64 = Wd.astype(np.float64), S.astype(np.float64)
    assert np.all(np.abs(Y - W64 @ S64) <= (n + 1) * 2.0 ** -24 * (np.abs(W64) @ np.abs(S64)))
    return Y


@functools.lru_cache(maxsize=None)
def problem(n, P, with_g=True):
    """(Wd, X0, [G per round], [X after round 1, 2, 3]): built once, shared, never modified.  Wd is
    not symmetric, so a transposed fragment fails."""
    rng = np.random.default_rng(n * 7 + P)
    Wd = (rng.standard_normal((n, n)) / n).astype(np.float32)
    X0 = rng.standard_normal((n, P), dtype=np.float32)
    Gs = [rng.standard_normal((n, P), dtype=np.float32) if with_g else None for _ in range(ROUNDS)]
    want, X = [], X0
    for G in Gs:
        X = rule(Wd, X, G, LR)
        want.append(X)
    for a in [Wd, X0] + Gs + want:
        if a is not None:
            a.setflags(write=False)
    return Wd, X0, Gs, want


def padded(a, cuda, aligned=False, fill=-7.5):
    """A row-major device buffer of ld = P + 3 (aligned: the next multiple of 4 above it, which
    the float4 kernel takes) filled with a sentinel, and its [n, P] view."""
    ld = a.shape[1] + 3 if not aligned else (a.shape[1] + 7) // 4 * 4
    buf = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=cuda)
    view = buf[:, :a.shape[1]]
    view.copy_(dev_t(a, cuda))
    return buf, view


@pytest.mark.parametrize("aligned", [False, True])   # the guarded kernel; float4 tiles + a tail
@pytest.mark.parametrize("with_g", [True, False])
@pytest.mark.parametrize("n,P", SHAPES)
def test_bits_match_the_fma_chain(cuda, n, P, with_g, aligned):
    Wd, X0, Gs, want = problem(n, P, with_g)
    W = dev_t(Wd, cuda)
    (xb, x), (yb, y) = padded(X0, cuda, aligned), padded(X0 * 0, cuda, aligned)
    for i, G in enumerate(Gs):
        gb, g = padded(G, cuda, aligned) if with_g else (None, None)
        E().dense_round(W, x, y, g, LR if with_g else 0.0)
        torch.cuda.synchronize()
        same(y.cpu().numpy(), want[i], f"y, round {i + 1}")
        for b in (xb, yb) + ((gb,) if with_g else ()):
            assert torch.all(b[:, P:] == -7.5), "the padding past n_params was written"
        (xb, x), (yb, y) = (yb, y), (xb, x)


def test_a_permutation_matrix_copies_rows_exactly(cuda):
    n, P = 100, 777
    rng = np.random.default_rng(11)
    perm = rng.permutation(n)
    X, G = (rng.standard_normal((n, P), dtype=np.float32) for _ in range(2))
    Wd = np.zeros((n, n), np.float32)
    Wd[np.arange(n), perm] = 1.0
    y = torch.empty(n, P, device=cuda)
    E().dense_round(dev_t(Wd, cuda), dev_t(X, cuda), y, dev_t(G, cuda), LR)
    same(y.cpu().numpy(), (X - np.float32(LR) * G)[perm], "y")


def test_the_tile_walk(cuda):
    """The smallest N with the smallest P at which workgroups walk more than one tile: float4
    tiles (rows of P + 3 floats, a multiple of 4) with a ragged tail tile behind them."""
    from distributed_learning_amd import _lib
    n, big = 32, _lib.DlMixPlan()
    # dummy addresses, never dereferenced: the saturated grid and the tile width for this N
    args = _lib.DlDenseRoundArgs(1 << 32, 1 << 24, 1 << 40, 1 << 24, None, 0, 0.0, 1 << 20, n, n,
                                 1 << 24, 0)
    assert _lib.load().dl_dense_round_plan(args, big) == _lib.DL_OK
    P = big.grid * big.tile_cols + 1
    Wd, X0, Gs, want = problem(n, P)
    assert (P + 3) % 4 == 0
    W, (_, x), (yb, y), (_, g) = dev_t(Wd, cuda), padded(X0, cuda), padded(X0, cuda), \
        padded(Gs[0], cuda)
    plan = E().dense_round_plan(W, x, y, g)
    assert plan["n_tiles"] > plan["grid"] and plan["path"] == 6
    E().dense_round(W, x, y, g, LR)
    same(y.cpu().numpy(), want[0], "y")
    assert torch.all(yb[:, P:] == -7.5)


@pytest.mark.parametrize("n,P,tile_cols", [(64, 4096, None), (256, 777, None), (64, 1000, 16),
                                          (256, 1000, 128)])   # the last: two kernel tiles a data tile
def test_tiled_engine_round_dense(cuda, n, P, tile_cols):
    Wd, X0, Gs, want = problem(n, P)
    g = E().GossipEngine(regular_csr(n), P, device=cuda, X=dev_t(X0, cuda), layout="tiled",
                         tile_cols=tile_cols)
    W, mean = dev_t(Wd, cuda), torch.empty(P, device=cuda)
    for i, G in enumerate(Gs):
        g.round_dense(W, g.layout_like(dev_t(G, cuda)), LR, deviation=i == ROUNDS - 1,
                      mean=mean if i == ROUNDS - 1 else None)
    torch.cuda.synchronize()
    same(g.rows().cpu().numpy(), want[-1], "rows()")
    check_dev(want[-1], g.dev_sq.cpu().numpy(), float(g.dev_max.cpu()), mean.cpu().numpy())


def test_captured_steps_replay_eager_ones(cuda):   # 3 eager, 2 replayed
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    from distributed_learning_amd.workloads import MLPConsensusSGD
    n, b, lr = 6, 64, 0.1
    gen = torch.Generator(device=cuda).manual_seed(7)
    bann = BatchedANN(n, b, 64, 32, 10, device=cuda)
    X0 = 0.1 * torch.randn(n, bann.P, device=cuda, generator=gen)
    data = torch.randn(n, b, 64, device=cuda, generator=gen)
    labels = torch.randint(0, 10, (n, b), device=cuda, generator=gen, dtype=torch.int32)
    Wd = torch.full((n, n), 1.0 / n, device=cuda)

    def trainer(**kw):
        g = E().GossipEngine(regular_csr(n), bann.P, device=cuda, X=X0)
        return g, MLPConsensusSGD(bann, g, data, labels, lr=lr, dense=Wd, **kw)
    (g, sgd), (h, hand) = trainer(), trainer()
    for i in range(5):
        if i == 3:
            torch.cuda.synchronize()
            assert torch.equal(g.X, h.X) and not torch.equal(g.rows(), X0)
            sgd.capture()
        sgd.replay() if i >= 3 else sgd.step()
        hand.gradients()
        h.round_dense(Wd, hand.G, lr, deviation=True)
    torch.cuda.synchronize()
    assert torch.equal(g.X, h.X) and torch.equal(g.dev_sq, h.dev_sq)
    with pytest.raises(ValueError):
        trainer(trim=1)


def test_dense_power_is_k_rounds(cuda):
    """One round with W^5 against five rounds with W on the ring of 8 with its FDLA weight: five
    left folds of three terms, rows summing to 1 in magnitude <= 1, so both lie within 5 (3 + 2)
    2^-24 max|X| of each other and of the fp64 W^5 X."""
    from distributed_learning_amd.graph import Csr
    n, P, k = 8, 64, 5
    w = 1 / (3 - np.cos(2 * np.pi / n))
    cols = np.concatenate([[a, (a + 1) % n, (a - 1) % n] for a in range(n)])
    csr = Csr(np.arange(0, 3 * n + 1, 3), cols, np.tile([1 - 2 * w, w, w], n))
    X0 = np.random.default_rng(5).standard_normal((n, P), dtype=np.float32)
    one, five = (E().GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda), layout="rows")
                 for _ in range(2))
    one.round_dense(one.dense_power(k))
    for _ in range(k):
        five.round()
    torch.cuda.synchronize()
    got, ref = one.rows().cpu().numpy().astype(np.float64), five.rows().cpu().numpy()
    bound = k * (3 + 2) * 2.0 ** -24 * np.abs(X0).max()
    exact = np.linalg.matrix_power(csr.dense(), k) @ X0.astype(np.float64)
    assert np.abs(got - ref).max() <= bound and np.abs(got - exact).max() <= bound
