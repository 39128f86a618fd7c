"""GPU parity of the trimmed-mean round (dl_trim_round) with its rule (include/dlamd.h), restated
in numpy below, bit for bit; its deviation, resilience, capture and the training loop."""
import functools

import numpy as np
import pytest
import torch

from test_mix_gpu import check_dev
from test_sgd_round_gpu import FAMILIES, LR, dev_t, family_params, problem, regular_csr, same

pytestmark = pytest.mark.gpu
ROUNDS = 3


def E():
    from distributed_learning_amd import engine
    return engine


def rule(csr, X, b, G=None, lr=0.0):
    """One round of the rule in fp32, held to (k + 2) 2^-24 (sum |kept| + |self|) / (k + 1) of
    an fp64 evaluation of the same kept values: k + 1 roundings and one of margin."""
    S = X if G is None else X - np.float32(lr) * G
    Y = np.empty_like(S)
    with np.errstate(invalid="ignore"):
        for a in range(len(S)):
            cols = csr.col[csr.rowptr[a]:csr.rowptr[a + 1]]
            nb = cols[cols != a]
            u = np.sort(S[nb], axis=0)[b:len(nb) - b]
            acc = np.zeros(S.shape[1], np.float32)
            for row in u:
                acc = acc + row
            Y[a] = (acc + S[a]) / np.float32(len(nb) - 2 * b + 1)
            u64, k = u.astype(np.float64), len(u)
            exact = (u64.sum(axis=0) + S[a]) / (k + 1)
            bound = (k + 2) * 2.0 ** -24 * (np.abs(u64).sum(axis=0) + np.abs(S[a])) / (k + 1)
            ok = np.isfinite(exact)
            assert np.all(np.abs(Y[a].astype(np.float64) - exact)[ok] <= bound[ok]), a
    return Y


def operands(n, P, deg, plant=False):
    """test_sgd_round_gpu's problem (the circulant at 64 x deg 4); plant: +-Inf, -0.0, +0.0."""
    csr, X0, Gs = problem(n, P, deg, "regular" if (n, deg) == (64, 4) else "random")
    if plant:
        X0 = X0.copy()
        X0[5, 10], X0[7, 20] = np.inf, -np.inf
        X0[9, 30:40], X0[11, 30:40] = -0.0, 0.0
    return csr, X0, Gs


@functools.lru_cache(maxsize=None)
def oracle(n, P, deg, b, with_g, plant=False):
    csr, X, Gs = operands(n, P, deg, plant)
    out = []
    for i in range(ROUNDS):
        X = rule(csr, X, b, Gs[i] if with_g else None, LR)
        out.append(X)
    return out


def run_rounds(cuda, csr, X0, Gs, b, in_place=False, ld=None, sentinel=0.0, dev=False,
               rounds=ROUNDS):
    """Row-major rounds at row stride ld: ([y per round], last deviation, the padded buffers)."""
    n, P = X0.shape
    W = E().DeviceCsr(csr, cuda)

    def padded(a=None):
        t = torch.full((n, ld or P), sentinel, device=cuda)
        t[:, :P] = dev_t(a, cuda) if a is not None else 0.0
        return t
    Xb, Yb = padded(X0), padded()
    Gb = [padded(g) for g in Gs] if Gs is not None else None
    devs = [torch.empty(k, device=cuda) for k in (n, 1, P)] if dev else [None] * 3
    out = []
    for i in range(rounds):
        Y = Xb if in_place else Yb
        assert E().trim_round(W, Xb[:, :P], Y[:, :P], Gb[i][:, :P] if Gb else None, LR, b,
                              dev_sq=devs[0], dev_max=devs[1], mean=devs[2]) is True
        if not in_place:
            Xb, Yb = Yb, Xb
        torch.cuda.synchronize()
        out.append(Xb[:, :P].cpu().numpy())
    if dev:
        devs = (devs[0].cpu().numpy(), float(devs[1].item()), devs[2].cpu().numpy())
    return out, devs, [Xb, Yb] + (Gb or [])


@pytest.mark.parametrize("n,P,deg,b,plant", [
    (2, 7, 1, 0, False),
    (33, 129, 4, 1, False),           # rows not 16-byte aligned: the guarded kernel
    (64, 4096, 4, 1, False),          # regular circulant: 4 slots, constant neighbour count
    (300, 777, 8, 3, True), (300, 777, 8, 0, False),          # rows of 7..8 neighbours: 8 slots
    (128, 3 * 128 + 5, 16, 7, False), (128, 3 * 128 + 5, 16, 2, False),   # 15..16: 16 slots
    (1024, 4100, 4, 1, False),        # 8 rows per thread
    (1500, 64, 6, 2, False)])
def test_bits_match_the_rule(cuda, n, P, deg, b, plant):
    csr, X0, Gs = operands(n, P, deg, plant)
    for with_g in (True, False):
        want = oracle(n, P, deg, b, with_g, plant)
        for in_place in (False, True):
            got, _, _ = run_rounds(cuda, csr, X0, Gs if with_g else None, b, in_place)
            for i in range(ROUNDS):
                same(got[i], want[i], f"y, round {i + 1}, g={with_g}, in place={in_place}")


@pytest.mark.parametrize("n,tiles,weights,dev", FAMILIES)
def test_kernel_families_and_the_walk(cuda, n, tiles, weights, dev):
    """2, 4, 8 rows a thread, full tiles and a ragged one, the walk; the padding survives."""
    P, b = family_params(tiles), 1
    csr, X0, Gs = problem(n, P, 4, weights)
    t = [torch.empty(n, P + 3, device=cuda)[:, :P] for _ in range(3)]
    plan = E().trim_round_plan(E().DeviceCsr(csr, cuda), t[0], t[1], t[2], trim=b, deviation=dev)
    assert plan["tile_cols"] == 128 and plan["n_tiles"] >= tiles, plan
    assert tiles == 3 or plan["grid"] < tiles, plan   # a workgroup walks more than one tile
    got, devs, bufs = run_rounds(cuda, csr, X0, Gs, b, ld=P + 3, sentinel=-7.25, dev=dev, rounds=2)
    same(got[1], rule(csr, rule(csr, X0, b, Gs[0], LR), b, Gs[1], LR), "y, round 2")
    assert all(torch.all(t[:, P:] == -7.25) for t in bufs)
    if dev:
        check_dev(got[-1], *devs)


@pytest.mark.parametrize("n,P,deg,b,weights", [(256, 1030, 4, 1, "regular"),   # no one-pass mean
                                               (300, 777, 8, 2, "random"),
                                               (1024, 4100, 4, 1, "random")])
def test_deviation(cuda, n, P, deg, b, weights):
    csr, X0, Gs = problem(n, P, deg, weights)
    assert bool(csr.doubly_stochastic) == (weights == "regular")
    got, devs, _ = run_rounds(cuda, csr, X0, Gs, b, dev=True, rounds=1)
    same(got[0], rule(csr, X0, b, Gs[0], LR), "y")
    check_dev(got[0], *devs)


@pytest.mark.parametrize("n,P,deg,b", [(64, 4096, 4, 1), (300, 777, 8, 2)])
def test_tiled_engine_round_trim(cuda, n, P, deg, b):
    csr, X0, Gs = operands(n, P, deg)
    g = E().GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda), layout="tiled")
    assert g.layout == "tiled" and g.order is None
    for i in range(ROUNDS):
        g.round_trim(g.layout_like(dev_t(Gs[i], cuda)), LR, trim=b)
    torch.cuda.synchronize()
    same(g.rows().cpu().numpy(), oracle(n, P, deg, b, True)[-1], "rows()")


@pytest.mark.parametrize("garbage", [1e30, -np.inf])
def test_one_bad_agent_moves_no_honest_one_out_of_range(cuda, garbage):
    n, P, bad = 64, 256, 17
    csr = regular_csr(n)
    X0 = np.random.default_rng(3).standard_normal((n, P), dtype=np.float32)
    X0[bad] = garbage
    got, _, _ = run_rounds(cuda, csr, X0, None, 1, rounds=1)
    Xd = dev_t(X0, cuda)
    Ym = torch.empty_like(Xd)
    E().mix_round(E().DeviceCsr(csr, cuda), Xd, Ym)
    plain, escaped = Ym.cpu().numpy(), False
    for a in set(range(n)) - {bad}:
        hood = [c for c in csr.col[csr.rowptr[a]:csr.rowptr[a + 1]] if c != bad]
        lo, hi = X0[hood].min(axis=0), X0[hood].max(axis=0)
        assert np.all((got[0][a] >= lo) & (got[0][a] <= hi)), a
        escaped |= bool(np.any(~((plain[a] >= lo) & (plain[a] <= hi))))
    assert escaped   # dl_mix_round on the same input does not stay in range


def test_two_captured_graphs_replay_four_eager_rounds(cuda):   # one graph per parity
    n, P, deg, b = 64, 4096, 4, 1
    csr, X0, Gs = operands(n, P, deg)

    def fresh():
        g = E().GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda))
        g.reserve_workspace(deviation=True)
        return g, g.layout_like(dev_t(Gs[0], cuda))
    e, Ge = fresh()
    for _ in range(4):
        e.round_trim(Ge, LR, trim=b, deviation=True)
    g, Gg = fresh()
    torch.cuda.synchronize()
    graphs = []
    for _ in range(2):
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            g.round_trim(Gg, LR, trim=b, deviation=True)
        graphs.append(cg)
    torch.cuda.synchronize()
    same(g.rows().cpu().numpy(), X0, "capture ran nothing")
    for i in range(4):
        graphs[i % 2].replay()
    torch.cuda.synchronize()
    assert torch.equal(g.X, e.X) and torch.equal(g.Y, e.Y)
    assert torch.equal(g.dev_sq, e.dev_sq) and torch.equal(g.dev_max, e.dev_max)


def test_mlp_consensus_sgd_steps_are_gradients_then_round_trim(cuda):   # 3 eager, 2 replayed
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    from distributed_learning_amd.workloads import MLPConsensusSGD
    n, b, lr = 6, 64, 0.1
    gen = torch.Generator(device=cuda).manual_seed(7)
    bann = BatchedANN(n, b, 64, 32, 10, device=cuda)
    X0 = 0.1 * torch.randn(n, bann.P, device=cuda, generator=gen)
    data = torch.randn(n, b, 64, device=cuda, generator=gen)
    labels = torch.randint(0, 10, (n, b), device=cuda, generator=gen, dtype=torch.int32)

    def trainer(**kw):
        g = E().GossipEngine(regular_csr(n), bann.P, device=cuda, X=X0)
        return g, MLPConsensusSGD(bann, g, data, labels, lr=lr, trim=1, **kw)
    (g, sgd), (h, hand) = trainer(), trainer()
    for i in range(5):
        if i == 3:
            torch.cuda.synchronize()
            assert torch.equal(g.X, h.X) and not torch.equal(g.rows(), X0)
            sgd.capture()
        sgd.replay() if i >= 3 else sgd.step()
        hand.gradients()
        h.round_trim(hand.G, lr, trim=1, deviation=True)
    torch.cuda.synchronize()
    assert torch.equal(g.X, h.X) and torch.equal(g.dev_sq, h.dev_sq)
    with pytest.raises(ValueError):
        trainer(tracking=True)


def test_engine_refusals(cuda, monkeypatch):
    from distributed_learning_amd.graph import Csr
    n, P = 64, 1000
    # row 9 without its diagonal; every row with 2b neighbours at b = 1
    ring = np.array([[a, (a + 1) % n, (a + 2) % n] for a in range(n)])
    nodiag = ring.copy()
    nodiag[9, 0] = 12
    for cols, row, text in ((nodiag, 9, "diagonal"), (ring, 0, "neighbours")):
        csr = Csr(np.arange(0, 3 * n + 1, 3), cols.ravel(), np.full(3 * n, 1 / 3))
        with pytest.raises(ValueError, match=f"{text}.*row {row} "):
            E().GossipEngine(csr, P, device=cuda).round_trim(trim=1)
    for knob, path, shape in (("DLAMD_FORCE_GATHER", 2, (regular_csr(n), P, cuda, None, "rows")),
                              ("DLAMD_FORCE_REG", 4, (regular_csr(1500), 64, cuda))):
        monkeypatch.setenv(knob, "1")
        g = E().GossipEngine(*shape)
        assert g.plan()["path"] == path
        with pytest.raises(RuntimeError, match=f"plan path 1.*this round plans path {path}"):
            g.round_trim(trim=1)
        monkeypatch.delenv(knob)
