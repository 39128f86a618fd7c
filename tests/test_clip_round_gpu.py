"""GPU checks of the per-edge distance pass (dl_edge_sqdist) against fp64, of dl_clip_weights and
GossipEngine.round_clip against their rules (include/dlamd.h) restated in numpy bit for bit, and
of the round's resilience, capture and training loop."""
import numpy as np
import pytest
import torch

from distributed_learning_amd import engine as E
from oracle import cref
from test_mix_gpu import check_dev
from test_sgd_round_gpu import LR, dev_t, problem, regular_csr, same

pytestmark = pytest.mark.gpu
# (n, P, degree, weights); the last: a workgroup walks several tiles (8 rows a thread), then a
# ragged tile of 4 columns
SHAPES = [(2, 7, 1, "random"), (33, 129, 4, "random"), (64, 4096, 4, "regular"),
          (300, 777, 8, "random"), (128, 389, 16, "random"), (1024, 4100, 4, "random"),
          (1500, 64, 6, "random"), (256, 256 * 128 + 4, 4, "random")]


def sqdist64(csr, S):
    """E in float64 from the fp32 s: exact differences, squared and summed in float64."""
    S64 = S.astype(np.float64)
    return np.concatenate([((S64[csr.col[csr.rowptr[a]:csr.rowptr[a + 1]]] - S64[a]) ** 2).sum(1)
                           for a in range(csr.n_rows)])


def clip_rule(csr, Esq, tau=None, drop=0):
    """dl_clip_weights in numpy fp32: (W', the radii)."""
    w = csr.w.astype(np.float32)
    out, taus = w.copy(), np.empty(csr.n_rows, np.float32)
    for a in range(csr.n_rows):
        e = np.arange(csr.rowptr[a], csr.rowptr[a + 1])
        off, dg = e[csr.col[e] != a], e[csr.col[e] == a][0]
        taus[a] = tau[a] if tau is not None else np.sqrt(np.sort(Esq[off])[::-1][drop])
        d = np.sqrt(Esq[off])
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(d == 0, np.float32(1), np.minimum(np.float32(1), taus[a] / d))
        out[off] = w[off] * c.astype(np.float32)
        acc = w[dg]
        for k in off:
            acc = np.float32(acc + np.float32(w[k] - out[k]))
        out[dg] = acc
    return out, taus


@pytest.mark.parametrize("n,P,deg,weights", SHAPES)
def test_distances_against_fp64(cuda, n, P, deg, weights):
    csr, X0, Gs = problem(n, P, deg, weights)
    W = E.DeviceCsr(csr, cuda)
    diag = csr.col == np.repeat(np.arange(n), np.diff(csr.rowptr))
    for G in (Gs[0], None):
        want = sqdist64(csr, X0 if G is None else X0 - np.float32(LR) * G)
        # row-major at a row stride of P + 4 with a sentinel in the padding, then column-tiled
        bufs = [torch.full((n, P + 4), -7.25, device=cuda) for _ in range(2)]
        bufs[0][:, :P], bufs[1][:, :P] = dev_t(X0, cuda), dev_t(Gs[0], cuda)
        runs = [(bufs[0][:, :P], bufs[1][:, :P] if G is not None else None, None)]
        g = E.GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda), layout="tiled")
        runs.append((g.X, g.layout_like(dev_t(G, cuda)) if G is not None else None, (P, g.T)))
        for Xd, Gd, tiled in runs:
            got = E.edge_sqdist(W, Xd, Gd, LR, tiled=tiled)
            assert got is not False, E._lib.load().dl_last_error()
            again = E.edge_sqdist(W, Xd, Gd, LR, tiled=tiled).cpu().numpy()
            got = got.cpu().numpy()
            assert np.all(np.abs(got - want)[~diag] <= (P + 3) * 2.0 ** -24 * want[~diag])
            assert np.all(got[diag] == 0) and not np.any(np.signbit(got[diag]))
            same(again, got, "a second call")
        assert all(torch.all(b[:, P:] == -7.25) for b in bufs)


@pytest.mark.parametrize("setting", ["tau", "inf", "drop1", "drop3"])
def test_clip_weights_bit_for_bit(cuda, setting):
    n, P, deg = 300, 777, 8
    csr, X0, _ = problem(n, P, deg)
    W = E.DeviceCsr(csr, cuda)
    Ed = E.edge_sqdist(W, dev_t(X0, cuda))
    Esq = Ed.cpu().numpy()
    off = csr.col != np.repeat(np.arange(n), np.diff(csr.rowptr))
    tau, drop = None, 0
    if setting == "tau":      # the median distance: some entries clip and some do not
        tau = np.full(n, np.sqrt(np.median(Esq[off])), np.float32)
    elif setting == "inf":
        tau = np.full(n, np.inf, np.float32)
    else:
        drop = int(setting[4:])
    want_w, want_tau = clip_rule(csr, Esq, tau, drop)
    out_w, tau_out = torch.empty_like(W.w), torch.empty(n, device=cuda)
    E.clip_weights(W, Ed, out_w, tau=dev_t(tau, cuda) if tau is not None else None, drop=drop,
                   tau_out=tau_out)
    same(out_w.cpu().numpy(), want_w, "W'")
    same(tau_out.cpu().numpy(), want_tau, "tau_out")
    clipped = np.mean(want_w[off] != csr.w.astype(np.float32)[off])
    assert clipped == 0 if setting == "inf" else 0 < clipped < 1, clipped
    if setting == "inf":
        same(want_w, csr.w.astype(np.float32), "W' at tau = +inf")


@pytest.mark.parametrize("layout", ["rows", "tiled"])
@pytest.mark.parametrize("n,P,deg,weights", SHAPES[:7])
def test_round_bits(cuda, n, P, deg, weights, layout):
    csr, X0, Gs = problem(n, P, deg, weights)
    # the two agents of the smallest graph have no neighbour to drop: a radius instead
    how = dict(drop=1) if n > 2 else dict(tau=1.0)
    for with_g in (True, False):
        g, twin, plain = [E.GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda), layout=layout)
                          for _ in range(3)]
        mean, X = torch.empty(P, device=cuda), X0
        for i in range(3):
            Gd = g.layout_like(dev_t(Gs[i], cuda)) if with_g else None
            g.round_clip(Gd, LR, deviation=True, mean=mean, **how)
            twin.round_clip(Gd, LR, tau=np.inf)
            plain.round(Gd, LR)
            torch.cuda.synchronize()
            # dl_mix_round's restatement, fed the device's weights
            X = cref.mix_round(X - np.float32(LR) * Gs[i] if with_g else X, csr.rowptr, csr.col,
                               g.Wc.w.cpu().numpy())
            same(g.rows().cpu().numpy(), X, f"x, round {i + 1}, g={with_g}")
            assert torch.equal(twin.X, plain.X), (i, with_g)
        check_dev(X, g.dev_sq.cpu().numpy(), float(g.dev_max.item()), mean.cpu().numpy())


@pytest.mark.parametrize("garbage", [1e15, 1e30])   # E finite, and E = +Inf
def test_one_bad_agent_moves_an_honest_one_by_at_most_its_radius(cuda, garbage):
    n, P, bad = 64, 256, 17
    csr = regular_csr(n)
    X0 = np.random.default_rng(3).standard_normal((n, P), dtype=np.float32)
    X0[bad] = garbage
    g = E.GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda), layout="rows")
    g.round_clip(drop=1)
    Ym = torch.empty_like(g.X)
    E.mix_round(g.W, dev_t(X0, cuda), Ym)
    y, plain = g.X.cpu().numpy().astype(np.float64), Ym.cpu().numpy().astype(np.float64)
    tau, wc = g.clip_tau.cpu().numpy().astype(np.float64), g.Wc.w.cpu().numpy().astype(np.float64)
    assert np.isinf(g.edge_sq.cpu().numpy()).any() == (garbage == 1e30)
    S, escaped = X0.astype(np.float64), False
    for a in set(range(n)) - {bad}:
        e = np.arange(csr.rowptr[a], csr.rowptr[a + 1])
        off = e[csr.col[e] != a]
        R = (len(e) + 3) * 2.0 ** -24 * np.linalg.norm(np.abs(wc[e]) @ np.abs(S[csr.col[e]]))
        bound = tau[a] * np.abs(csr.w[off]).sum() + R
        assert np.linalg.norm(y[a] - S[a]) <= bound, a
        escaped |= bad in csr.col[e] and np.linalg.norm(plain[a] - S[a]) > bound
    assert escaped   # dl_mix_round on the same input breaks the bound next to the bad agent


def test_two_captured_graphs_replay_four_eager_rounds(cuda):   # one graph per parity
    n, P, deg = 64, 4096, 4
    csr, X0, Gs = problem(n, P, deg, "regular")

    def fresh():
        g = E.GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda))
        g.reserve_workspace(deviation=True, clip=True)
        return g, g.layout_like(dev_t(Gs[0], cuda))
    e, Ge = fresh()
    for _ in range(4):
        e.round_clip(Ge, LR, drop=1, deviation=True)
    g, Gg = fresh()
    torch.cuda.synchronize()
    graphs = []
    for _ in range(2):
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            g.round_clip(Gg, LR, drop=1, deviation=True)
        graphs.append(cg)
    torch.cuda.synchronize()
    same(g.rows().cpu().numpy(), X0, "capture ran nothing")
    for i in range(4):
        graphs[i % 2].replay()
    torch.cuda.synchronize()
    for f in ("X", "Y", "dev_sq", "dev_max", "edge_sq", "clip_tau"):
        assert torch.equal(getattr(g, f), getattr(e, f)), f


def test_mlp_consensus_sgd_steps_are_gradients_then_round_clip(cuda):   # 3 eager, 2 replayed
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    from distributed_learning_amd.workloads import MLPConsensusSGD
    n, b, lr = 6, 64, 0.1
    gen = torch.Generator(device=cuda).manual_seed(7)
    bann = BatchedANN(n, b, 64, 32, 10, device=cuda)
    X0 = 0.1 * torch.randn(n, bann.P, device=cuda, generator=gen)
    data = torch.randn(n, b, 64, device=cuda, generator=gen)
    labels = torch.randint(0, 10, (n, b), device=cuda, generator=gen, dtype=torch.int32)

    def trainer(**kw):
        g = E.GossipEngine(regular_csr(n), bann.P, device=cuda, X=X0)
        return g, MLPConsensusSGD(bann, g, data, labels, lr=lr, clip=1, **kw)
    (g, sgd), (h, hand) = trainer(), trainer()
    for i in range(5):
        if i == 3:
            torch.cuda.synchronize()
            assert torch.equal(g.X, h.X) and not torch.equal(g.rows(), X0)
            sgd.capture()
        sgd.replay() if i >= 3 else sgd.step()
        hand.gradients()
        h.round_clip(hand.G, lr, drop=1, deviation=True)
    torch.cuda.synchronize()
    assert torch.equal(g.X, h.X) and torch.equal(g.dev_sq, h.dev_sq)
    for kw in (dict(trim=1), dict(tracking=True)):
        with pytest.raises(ValueError):
            trainer(**kw)


def test_engine_refusals(cuda, monkeypatch):
    from distributed_learning_amd.graph import Csr
    n, P = 64, 1000
    # row 9 without its diagonal; every row with 2 neighbours at drop = 2
    ring = np.array([[a, (a + 1) % n, (a + 2) % n] for a in range(n)])
    nodiag = ring.copy()
    nodiag[9, 0] = 12
    for cols, row, text in ((nodiag, 9, "diagonal"), (ring, 0, "neighbours")):
        csr = Csr(np.arange(0, 3 * n + 1, 3), cols.ravel(), np.full(3 * n, 1 / 3))
        with pytest.raises(ValueError, match=f"{text}.*row {row} "):
            E.GossipEngine(csr, P, device=cuda).round_clip(drop=2)
    monkeypatch.setenv("DLAMD_FORCE_GATHER", "1")
    g = E.GossipEngine(regular_csr(n), P, cuda, None, "rows")
    assert g.plan()["path"] == 2
    with pytest.raises(RuntimeError, match="plan path 1.*this round plans path 2"):
        g.round_clip(drop=1)
