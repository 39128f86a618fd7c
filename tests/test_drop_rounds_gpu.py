"""GPU parity of dl_drop_rounds (GossipEngine.rounds_drop) with its rule restated in numpy fp32:
the hash of test_drop_rounds_abi.py and the fold -- wd = w[e0] + the down entries' weights, then
from +0.0 wd x_i and w[e] x_col[e] for the up entries, in CSR order.  Bit for bit, NaN-aware.  Five
rounds from round 7 per (graph, step, probabilities) serve every K, layout and split."""
import functools

import numpy as np
import pytest
import torch

from test_drop_rounds_abi import up_mask
from test_mix_gpu import DEV_RTOL, bits, dev_floor, shared_weight_graph

pytestmark = pytest.mark.gpu

SEED, R0, LR = 3, 7, 0.05
PROBS = [(0.0, 0.0), (0.3, 0.0), (0.3, 0.2), (1.0, 0.0)]


@functools.lru_cache(maxsize=None)
def graph(name):
    """(csr, column-tiled width, columns).  At 64 columns a thread holds 1 (64 agents), 2 ragged
    (100) or 4 (256) rows; the *T4 graphs run 600 tiles of 4 columns, more than workgroups."""
    from distributed_learning_amd import graph as G
    kind, n = name[:3], int(name[3:].split("T")[0])
    T = 4 if name.endswith("T4") else 64
    P = 4 * 600 if T == 4 else 192
    if kind == "reg":     # 4-regular, shared weights: the register CSR
        return shared_weight_graph(n, seed=n), T, P
    if kind == "tor":     # the c4 shape's 64 x 64 torus: 4 rows a thread at 4 columns
        e = G.torus_edges(64, 64)
        return G.from_edge_weights(e, [0.2] * len(e), list(range(n))), T, P
    # irregular, Metropolis weights: agent 0 a hub of n - 2 links, agents 1 .. n - 2 on a ring,
    # agent n - 1 alone (a self-only row)
    e = [(0, j) for j in range(1, n - 1)] + [(j, j + 1) for j in range(1, n - 2)] + [(n - 2, 1)]
    deg = np.bincount(np.array(e).ravel(), minlength=n)
    return G.from_edge_weights(e, [1.0 / (1 + max(deg[i], deg[j])) for i, j in e],
                               list(range(n))), T, P


def inputs(name):
    csr, _, P = graph(name)
    rng = np.random.default_rng(11)
    return (rng.standard_normal((csr.n_rows, P), dtype=np.float32),
            rng.standard_normal((csr.n_rows, P), dtype=np.float32))


def drop_round(csr, X, up):
    rp, col, w = csr.rowptr, csr.col, np.asarray(csr.w, np.float32)
    out = np.empty_like(X)
    with np.errstate(invalid="ignore"):
        for a in range(csr.n_rows):
            e0, e1 = rp[a], rp[a + 1]
            wd = w[e0]
            for e in range(e0 + 1, e1):
                if not up[e]:
                    wd = wd + w[e]
            acc = np.zeros(X.shape[1], np.float32) + wd * X[col[e0]]
            for e in range(e0 + 1, e1):
                if up[e]:
                    acc = acc + w[e] * X[col[e]]
            out[a] = acc
    return out


@functools.lru_cache(maxsize=None)
def sequence(name, sgd, probs, inf_row=None):
    """[x after k rounds for k = 0 .. 5], rounds R0, R0 + 1, ..."""
    csr = graph(name)[0]
    X, G = inputs(name)
    if inf_row is not None:
        X = X.copy()
        X[inf_row] = np.inf
    u = [X - np.float32(LR) * G if sgd else X]
    for t in range(R0, R0 + 5):
        u.append(drop_round(csr, u[-1], up_mask(csr, SEED, t, *probs)))
    return u


def engine(cuda, name, layout, X=None):
    from distributed_learning_amd import engine as E
    csr, T, P = graph(name)
    X = inputs(name)[0] if X is None else X
    return E.GossipEngine(csr, P, device=cuda, X=torch.from_numpy(X).to(cuda), layout=layout,
                          tile_cols=T if layout == "tiled" else None, order=None)


def same(eng, want, what):
    assert np.array_equal(bits(eng.rows().cpu().numpy()), bits(want)), what


@pytest.mark.parametrize("sgd", [False, True])
@pytest.mark.parametrize("layout", ["tiled", "rows"])
@pytest.mark.parametrize("name", ["irr64", "irr100", "irr256", "reg100", "reg256"])
def test_passes_match_the_restatement(cuda, name, layout, sgd):
    for probs in PROBS:
        u = sequence(name, sgd, probs)
        for K in (1, 2, 5):
            eng = engine(cuda, name, layout)
            G = eng.layout_like(torch.from_numpy(inputs(name)[1])) if sgd else None
            eng.rounds_drop(K, *probs, seed=SEED, round0=R0, G=G, lr=LR, deviation=K == 5)
            same(eng, u[K], (probs, K))
            if K == 5:   # the bar of dl_mix_rounds' deviation (test_mix_gpu.check_dev)
                y = u[K].astype(np.float64)
                tol = dict(rtol=DEV_RTOL, atol=dev_floor(y.mean(0), y.shape[1]))
                want = np.sqrt(((y - y.mean(0)) ** 2).sum(1))
                np.testing.assert_allclose(np.sqrt(eng.dev_sq.cpu().numpy()), want, **tol)
                np.testing.assert_allclose(eng.dev_max.item(), want.max(), **tol)
            if probs == (0.0, 0.0):   # no link down: dl_mix_rounds' bits
                ref = engine(cuda, name, layout)
                ref.rounds(K, G=G, lr=LR)
                same(eng, ref.rows().cpu().numpy(), ("rounds", K))


@pytest.mark.parametrize("name", ["reg64T4", "tor4096T4"])
def test_more_tiles_than_workgroups(cuda, name):
    from distributed_learning_amd import engine as E
    eng = engine(cuda, name, "tiled")
    plan = E.drop_rounds_plan(eng.W, eng.X, eng.Y, tiled=(eng.P, eng.T))
    assert plan["n_tiles"] > plan["grid"], plan
    eng.rounds_drop(2, 0.3, 0.2, seed=SEED, round0=R0, lr=LR,
                    G=eng.layout_like(torch.from_numpy(inputs(name)[1])))
    same(eng, sequence(name, True, (0.3, 0.2))[2], name)


def test_split_passes_and_the_device_counter(cuda):
    u = sequence("irr100", False, (0.3, 0.2))
    eng = engine(cuda, "irr100", "tiled")
    eng.rounds_drop(2, 0.3, 0.2, seed=SEED, round0=R0)
    eng.rounds_drop(3, 0.3, 0.2, seed=SEED, round0=R0 + 2)
    same(eng, u[5], "2 + 3 rounds")
    eng = engine(cuda, "irr100", "tiled")   # the engine's counter: set to R0, advanced by K
    eng.drop_round = torch.full((1,), R0, dtype=torch.int32, device=cuda)
    for K, done in ((2, 2), (3, 5)):
        eng.rounds_drop(K, 0.3, 0.2, seed=SEED)
        assert eng.drop_round.item() == R0 + done
        same(eng, u[done], ("counter", done))


@pytest.mark.parametrize("name", ["irr100", "reg100"])
def test_a_down_neighbours_inf_stays_out(cuda, name):
    csr, bad = graph(name)[0], 1
    u = sequence(name, False, (0.3, 0.0), inf_row=bad)
    eng = engine(cuda, name, "tiled", X=u[0])
    eng.rounds_drop(1, 0.3, 0.0, seed=SEED, round0=R0)
    got = eng.rows().cpu().numpy()
    assert np.array_equal(bits(got), bits(u[1]))
    up = up_mask(csr, SEED, R0, 0.3, 0.0)
    row = np.repeat(np.arange(csr.n_rows), np.diff(csr.rowptr))
    hit = np.zeros(csr.n_rows, bool)
    hit[row[(np.asarray(csr.col) == bad) & up]] = True   # rows that read agent `bad` this round
    assert hit.sum() > 1 and (~hit).sum() > 1 and ((np.asarray(csr.col) == bad) & ~up).any()
    assert np.isfinite(got[~hit]).all() and np.isinf(got[hit]).all()
