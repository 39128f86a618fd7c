"""GPU parity of the gradient-tracking round (dl_track_round) with its definition
(track_oracle.track_step: fp32 numpy element-wise operations around the oracle's fold) -- three
consecutive rounds with a distinct gradient per step and the previous one as g_old, x' and d'
in place or apart.  The rounds are bit-exact in X and D, deviations within 1e-5 relative; the
composed three-launch form gives the same bits; on quadratic losses the tracked iterates reach
the optimum where the plain round stalls (test_tracking_host.py pins that on the CPU)."""
import functools

import numpy as np
import pytest
import torch

import track_oracle as O
from oracle import cref
from test_mix_gpu import DEV_RTOL, check_dev, graph_csr
from test_sgd_round_gpu import FAMILIES, SHAPES, dev_t, family_params, problem, same

pytestmark = pytest.mark.gpu

LR = 0.05
ROUNDS = 3
# x' apart + d' = d (the engine's mode), both in place, both apart
MODES = ["d'=d", "x'=x,d'=d", "apart"]


def E():
    from distributed_learning_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def operands(n, P, deg, weights="random"):
    """(csr, X0, D0, Q0, [G per round]): test_sgd_round_gpu's problem, with a tracker and a last
    gradient unrelated to it, so that all four streams differ from the first round on."""
    csr, X0, Gs = problem(n, P, deg, weights)
    rng = np.random.default_rng(n * 11 + P)
    D0 = rng.standard_normal((n, P), dtype=np.float32)
    Q0 = rng.standard_normal((n, P), dtype=np.float32)
    D0.setflags(write=False)
    Q0.setflags(write=False)
    return csr, X0, D0, Q0, Gs


def oracle_rounds(csr, X, D, Q, Gs, lr=LR):
    out = []
    for G in Gs:
        X, D = O.track_step(csr, X, D, G, Q, lr)
        Q = G
        out.append((X, D))
    return out


@functools.lru_cache(maxsize=None)
def oracle(n, P, deg, weights="random"):
    """[(X, D) after round 1..ROUNDS]: the same for every aliasing mode."""
    return oracle_rounds(*operands(n, P, deg, weights))


def run_rounds(cuda, csr, X0, D0, Q0, Gs, mode, ld=None, sentinel=None, dev=False,
               composed=False):
    """len(Gs) rounds on row-major operands (ld: row stride, the padding filled with
    ``sentinel``).  Returns ([(X, D) per round], last (dev_sq, dev_max, mean), every padded
    buffer).  composed: (D + G) - Gold in torch, dl_mix_round of it, dl_mix_round with g = D'."""
    eng = E()
    n, P = X0.shape
    ld = ld or P
    W = eng.DeviceCsr(csr, cuda)

    def padded(a=None):
        t = torch.full((n, ld), sentinel if sentinel is not None else 0.0, device=cuda)
        t[:, :P] = dev_t(a, cuda) if a is not None else 0.0
        return t
    Xb, Yb, Db, Eb = padded(X0), padded(), padded(D0), padded()
    Gb = [padded(Q0)] + [padded(G) for G in Gs]
    dsq = torch.empty(n, device=cuda) if dev else None
    dmax = torch.empty(1, device=cuda) if dev else None
    mean = torch.empty(P, device=cuda) if dev else None
    v = lambda t: t[:, :P]   # noqa: E731
    if not composed:
        plan = eng.track_round_plan(W, v(Xb), v(Yb), v(Db), v(Db), v(Gb[1]), v(Gb[0]),
                                    deviation=dev)
        assert plan is not None and plan["path"] == 1
    out = []
    for i in range(len(Gs)):
        X, D, G, Q = v(Xb), v(Db), v(Gb[i + 1]), v(Gb[i])
        Y = X if mode == "x'=x,d'=d" else v(Yb)
        Dn = v(Eb) if mode == "apart" else D
        if composed:
            T = (D + G) - Q
            eng.mix_round(W, T, v(Eb))
            eng.mix_round(W, X, v(Yb), G=v(Eb), lr=LR, dev_sq=dsq, dev_max=dmax, mean=mean)
            Y, Dn = v(Yb), v(Eb)
        else:
            assert eng.track_round(W, X, Y, D, Dn, G, Q, LR, dev_sq=dsq, dev_max=dmax,
                                   mean=mean) is True
        if Y is not X:
            Xb, Yb = Yb, Xb
        if Dn is not D:
            Db, Eb = Eb, Db
        torch.cuda.synchronize()
        out.append((v(Xb).cpu().numpy(), v(Db).cpu().numpy()))
    devs = (dsq.cpu().numpy(), float(dmax.item()), mean.cpu().numpy()) if dev else None
    return out, devs, [Xb, Yb, Db, Eb] + Gb


def check_rounds(got, want, what):
    for i, ((x, d), (wx, wd)) in enumerate(zip(got, want)):
        same(d, wd, f"D, round {i + 1}, {what}")
        same(x, wx, f"X, round {i + 1}, {what}")


@pytest.mark.parametrize("n,P,deg", SHAPES)
def test_bits_match_the_definition_and_the_composed_form(cuda, n, P, deg):
    ops = operands(n, P, deg)
    want = oracle(n, P, deg)
    for mode in MODES:
        got, _, _ = run_rounds(cuda, *ops, mode)
        check_rounds(got, want, mode)
    comp, _, _ = run_rounds(cuda, *ops, "apart", composed=True)
    check_rounds(comp, want, "torch + two dl_mix_round")


@pytest.mark.parametrize("n,tiles,weights,dev", FAMILIES)
def test_kernel_families(cuda, n, tiles, weights, dev):
    """mix_track_tile_kernel's instantiation families (those of test_sgd_round_gpu.FAMILIES: the
    rounds are shaped alike): 2 / 4 / 8 rows per thread, five-weight and CSR rows, the mean from
    the staged s and the two-pass form, the tile walk, and a ragged 5-column tail on the guarded
    kernel, at ld = P + 3 with a sentinel in every operand's padding."""
    P, deg = family_params(tiles), 4
    ops = operands(n, P, deg, weights)
    want = oracle(n, P, deg, weights)
    t = [torch.empty(n, P + 3, device=cuda)[:, :P] for _ in range(5)]
    plan = E().track_round_plan(E().DeviceCsr(ops[0], cuda), t[0], t[1], t[2], t[2], t[3], t[4],
                                deviation=dev)
    assert plan["tile_cols"] == 128 and plan["n_tiles"] >= tiles, plan
    assert tiles == 3 or plan["grid"] < tiles, plan   # a workgroup walks more than one tile
    got, devs, bufs = run_rounds(cuda, *ops, "d'=d", ld=P + 3, sentinel=-7.25, dev=dev)
    check_rounds(got, want, "families")
    for b in bufs:
        assert torch.all(b[:, P:] == -7.25)
    if dev:
        check_dev(got[-1][0], *devs)


def test_workgroups_walk_three_tiles(cuda):
    """n_tiles >= 3 x grid (both from dl_track_round_plan): the cross-tile prefetch and the
    in-tile loads of x run more than once per workgroup; with a ragged tail tile behind the full
    ones."""
    eng = E()
    n, deg = 64, 4
    csr = graph_csr(n, deg, seed=5)
    W = eng.DeviceCsr(csr, cuda)

    def plan(P):
        t = [torch.empty(n, P, device=cuda) for _ in range(5)]
        return eng.track_round_plan(W, t[0], t[1], t[2], t[2], t[3], t[4])
    p0 = plan(1 << 20)
    P = 3 * p0["grid"] * p0["tile_cols"] + 4     # (rows stay 16-byte aligned: the float4 kernel)
    assert n * P * 4 <= 256 << 20
    p = plan(P)
    assert p is not None and p["path"] == 1 and p["n_tiles"] >= 3 * p["grid"], p
    assert P % p["tile_cols"] != 0
    rng = np.random.default_rng(1)
    X0, D0, Q0, G1, G2 = (rng.standard_normal((n, P), dtype=np.float32) for _ in range(5))
    want = oracle_rounds(csr, X0, D0, Q0, [G1, G2])
    for mode in ("d'=d", "x'=x,d'=d"):
        got, _, _ = run_rounds(cuda, csr, X0, D0, Q0, [G1, G2], mode)
        check_rounds(got[-1:], want[-1:], mode)


@pytest.mark.parametrize("n,P,deg,weights", [(256, 1030, 4, "regular"), (300, 777, 8, "random"),
                                             (1500, 64, 6, "random"), (64, 4096, 4, "regular"),
                                             (64, 4096, 4, "random"), (1024, 4100, 4, "random")])
def test_deviation(cuda, n, P, deg, weights):
    """dev_sq, dev_max and mean of x': one pass for a doubly stochastic W (uniform weights on a
    regular graph), two passes otherwise."""
    ops = operands(n, P, deg, weights)
    assert bool(ops[0].doubly_stochastic) == (weights == "regular")
    want = oracle(n, P, deg, weights)
    for mode in ("d'=d", "apart"):
        got, (dsq, dmax, mean), _ = run_rounds(cuda, *ops, mode, dev=True)
        check_rounds(got[-1:], want[-1:], mode)
        check_dev(got[-1][0], dsq, dmax, mean)


@pytest.mark.parametrize("mode", ["x'=x,d'=d", "apart"])
def test_unaligned_rows_take_the_guarded_kernel(cuda, mode):
    """33 x 129 at ld = P + 4 = 133: rows are not 16-byte aligned, so every tile runs the guarded
    kernel; sentinels in the padding of every operand survive."""
    n, P, deg = 33, 129, 4
    ops = operands(n, P, deg)
    got, devs, bufs = run_rounds(cuda, *ops, mode, ld=P + 4, sentinel=-7.25, dev=True)
    check_rounds(got, oracle(n, P, deg), mode)
    check_dev(got[-1][0], *devs)
    for b in bufs:
        assert torch.all(b[:, P:] == -7.25)


def engine_rounds(g, ops, deviation=True):
    """ROUNDS x round_track on engine g (X loaded) from the operands' tracker and gradients."""
    _, _, D0, Q0, Gs = ops
    g.D = g.layout_like(dev_t(D0, g.device))
    bufs = [g.layout_like(dev_t(a, g.device)) for a in [Q0] + list(Gs)]
    for i in range(len(Gs)):
        g.round_track(bufs[i + 1], bufs[i], LR, deviation=deviation)
    torch.cuda.synchronize()


def tracker_rows(g):
    return (E().from_tiled(g.D, g.P) if g.layout == "tiled" else g.D).cpu().numpy()


@pytest.mark.parametrize("n,P,deg", [(64, 4096, 4), (300, 777, 8)])
def test_tiled_engine_round_track(cuda, n, P, deg):
    """GossipEngine(layout="tiled").round_track: rows() and the un-tiled D are the row-major
    result's bits."""
    eng = E()
    ops = operands(n, P, deg)
    want = oracle(n, P, deg)
    g = eng.GossipEngine(ops[0], P, device=cuda, X=dev_t(ops[1], cuda), layout="tiled")
    assert g.layout == "tiled" and g.order is None
    g.reset_tracker()
    G, Q = g.layout_like(dev_t(ops[4][0], cuda)), g.layout_like(dev_t(ops[3], cuda))
    assert eng.track_round_plan(g.W, g.X, g.Y, g.D, g.D, G, Q, tiled=(P, g.T),
                                deviation=True) is not None
    engine_rounds(g, ops)
    same(g.rows().cpu().numpy(), want[-1][0], "rows()")
    same(tracker_rows(g), want[-1][1], "D")
    np.testing.assert_allclose(np.sqrt(g.dev_sq.cpu().numpy()),
                               np.sqrt(cref.deviation_sq(want[-1][0])), rtol=DEV_RTOL)


def test_fallback_when_the_plan_is_not_path_1(cuda, monkeypatch):
    monkeypatch.setenv("DLAMD_FORCE_GATHER", "1")
    eng = E()
    n, P, deg = 64, 1000, 4
    ops = operands(n, P, deg)
    g = eng.GossipEngine(ops[0], P, device=cuda, X=dev_t(ops[1], cuda), layout="rows")
    assert g.plan()["path"] == 2 and g.layout == "rows"
    g.reset_tracker()
    G, Q = g.layout_like(dev_t(ops[4][0], cuda)), g.layout_like(dev_t(ops[3], cuda))
    assert eng.track_round_plan(g.W, g.X, g.Y, g.D, g.D, G, Q) is None           # UNSUPPORTED
    assert eng.track_round(g.W, g.X, g.Y, g.D, g.D, G, Q, LR) is False
    engine_rounds(g, ops)
    want = oracle(n, P, deg)
    same(g.rows().cpu().numpy(), want[-1][0], "rows()")
    same(tracker_rows(g), want[-1][1], "D")
    np.testing.assert_allclose(np.sqrt(g.dev_sq.cpu().numpy()),
                               np.sqrt(cref.deviation_sq(want[-1][0])), rtol=DEV_RTOL)


def test_fallback_in_the_tiled_layout(cuda, monkeypatch):
    """Plan path 4 (the register-CSR kernel) keeps the tiled layout: torch forms (D + G) - Gold
    over the resident buffers, the plain rounds mix it and step along it."""
    monkeypatch.setenv("DLAMD_FORCE_REG", "1")
    eng = E()
    n, P = 1500, 64
    ops = operands(n, P, 4, "regular")
    g = eng.GossipEngine(ops[0], P, device=cuda, X=dev_t(ops[1], cuda))
    assert g.plan()["path"] == 4 and g.layout == "tiled"
    g.reset_tracker()
    G, Q = g.layout_like(dev_t(ops[4][0], cuda)), g.layout_like(dev_t(ops[3], cuda))
    assert eng.track_round_plan(g.W, g.X, g.Y, g.D, g.D, G, Q, tiled=(P, g.T)) is None
    assert eng.track_round(g.W, g.X, g.Y, g.D, g.D, G, Q, LR, tiled=(P, g.T)) is False
    engine_rounds(g, ops, deviation=False)
    want = oracle(n, P, 4, "regular")
    same(g.rows().cpu().numpy(), want[-1][0], "rows()")
    same(tracker_rows(g), want[-1][1], "D")


def test_captured_rounds_replay_the_eager_bits(cuda):
    """One graph per parity (X / Y and the two gradient buffers flip together); replayed
    alternately, four replays give the bits and the deviation of four eager rounds."""
    eng = E()
    n, P, deg = 64, 4096, 4
    csr, X0, D0, Q0, Gs = operands(n, P, deg)

    def fresh():
        g = eng.GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda))
        g.D = g.layout_like(dev_t(D0, cuda))
        g.reserve_workspace(deviation=True)
        return g, [g.layout_like(dev_t(Gs[0], cuda)), g.layout_like(dev_t(Q0, cuda))]
    e, eb = fresh()
    for i in range(4):
        e.round_track(eb[i % 2], eb[1 - i % 2], LR, deviation=True)
    torch.cuda.synchronize()
    g, gb = fresh()
    torch.cuda.synchronize()
    graphs = []
    for i in range(2):
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            g.round_track(gb[i], gb[1 - i], LR, deviation=True)
        graphs.append(cg)
    torch.cuda.synchronize()
    same(g.rows().cpu().numpy(), X0, "capture ran nothing (X)")
    same(tracker_rows(g), D0, "capture ran nothing (D)")
    for i in range(4):
        graphs[i % 2].replay()
    torch.cuda.synchronize()
    assert torch.equal(g.X, e.X) and torch.equal(g.D, e.D)
    assert torch.equal(g.dev_sq, e.dev_sq) and torch.equal(g.dev_max, e.dev_max)
    want = oracle_rounds(csr, X0, D0, Q0, [Gs[0], Q0, Gs[0], Q0])
    same(g.rows().cpu().numpy(), want[-1][0], "rows() after four replays")
    same(tracker_rows(g), want[-1][1], "D after four replays")


def test_quadratic_losses_end_to_end(cuda):
    """f_a(x) = 1/2 ||x - c_a||^2 on 64 agents of a random 4-regular graph, P = 16, 300 rounds at
    lr 0.1 from X = 0, the gradients X - C by torch (exact fp32): the final X is the oracle's bit
    for bit -- so within the 1e-4 of the optimum that test_tracking_host.py establishes -- and
    300 plain rounds from the same start stay more than 0.1 away."""
    eng = E()
    n, P, lr, rounds = 64, 16, 0.1, 300
    csr = O.uniform_regular_csr(n, 4, seed=0)
    c = O.quadratic_targets(n, P)
    want, want_d = O.tracked_run(csr, c, lr, rounds)
    assert O.distance(want, c) < 1e-4
    g = eng.GossipEngine(csr, P, device=cuda, X=torch.zeros(n, P, device=cuda))
    g.reset_tracker()
    C = g.layout_like(dev_t(c, cuda))
    G = [g.layout_like(torch.zeros(n, P, device=cuda)) for _ in range(2)]
    for i in range(rounds):
        torch.sub(g.X, C, out=G[i % 2])
        g.round_track(G[i % 2], G[1 - i % 2], lr)
    torch.cuda.synchronize()
    got = g.rows().cpu().numpy()
    same(got, want, "X after 300 tracked rounds")
    same(tracker_rows(g), want_d, "D after 300 tracked rounds")
    assert O.distance(got, c) < 1e-4
    g.load_rows(torch.zeros(n, P, device=cuda))
    for i in range(rounds):
        torch.sub(g.X, C, out=G[0])
        g.round(G[0], lr)
    torch.cuda.synchronize()
    plain = g.rows().cpu().numpy()
    same(plain, O.plain_run(csr, c, lr, rounds), "X after 300 plain rounds")
    assert O.distance(plain, c) > 0.1


def test_mlp_consensus_sgd_with_tracking(cuda):
    """MLPConsensusSGD(tracking=True) with BatchedANN, 4 agents x 64 samples on a ring: three
    eager steps are a hand-composed loop of ann.gradients into alternating buffers and
    engine.track_round; after one more eager step, capture() and two replay()s equal two further
    eager steps of a twin, bit for bit."""
    from distributed_learning_amd.graph import Csr
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    from distributed_learning_amd.workloads import MLPConsensusSGD
    eng = E()
    n, b, lr = 4, 64, 0.1
    cl = np.concatenate([[a, (a + 1) % n, (a - 1) % n] for a in range(n)])
    csr = Csr(np.arange(0, 3 * n + 1, 3), cl, np.full(cl.size, 1.0 / 3))
    gen = torch.Generator(device=cuda).manual_seed(7)
    bann = BatchedANN(n, b, 64, 32, 10, device=cuda)
    X0 = 0.1 * torch.randn(n, bann.P, device=cuda, generator=gen)
    data = torch.randn(n, b, 64, device=cuda, generator=gen)
    labels = torch.randint(0, 10, (n, b), device=cuda, generator=gen, dtype=torch.int32)

    def trainer():
        g = eng.GossipEngine(csr, bann.P, device=cuda, X=X0)
        return g, MLPConsensusSGD(bann, g, data, labels, lr=lr, tracking=True)
    g, sgd = trainer()
    assert sgd.tracking and torch.count_nonzero(g.D) == 0
    for _ in range(3):
        sgd.step()
    # the same three steps by hand
    h = eng.GossipEngine(csr, bann.P, device=cuda, X=X0)
    assert h.layout == g.layout
    tiled = (h.P, h.T) if h.layout == "tiled" else None
    D = torch.zeros_like(h.X)
    Gs = [torch.zeros_like(h.X), torch.zeros_like(h.X)]
    for i in range(3):
        if tiled:
            bann.gradients(h.X, data, labels, Gs[i % 2])
        else:
            bann.gradients(h.X[:, :bann.P], data, labels, Gs[i % 2][:, :bann.P])
        assert eng.track_round(h.W, h.X, h.Y, D, D, Gs[i % 2], Gs[1 - i % 2], lr,
                               dev_sq=h.dev_sq, dev_max=h.dev_max, workspace=h.ws,
                               tiled=tiled) is True
        h.X, h.Y = h.Y, h.X
    torch.cuda.synchronize()
    assert torch.equal(g.X, h.X) and torch.equal(g.D, D)
    assert torch.equal(g.dev_sq, h.dev_sq)
    assert not torch.equal(g.rows(), X0) and torch.count_nonzero(g.D) > 0
    # a twin runs six eager steps; this one four, then two replays
    t, twin = trainer()
    for _ in range(6):
        twin.step()
    sgd.step()
    sgd.capture()
    sgd.replay(2)
    torch.cuda.synchronize()
    assert sgd.steps_done == twin.steps_done == 6
    assert torch.equal(g.X, t.X) and torch.equal(g.D, t.D)
    assert torch.equal(g.dev_sq, t.dev_sq)
    for kw in (dict(momentum=0.9), dict(weight_decay=5e-4), dict(emit="step")):
        with pytest.raises(ValueError):
            MLPConsensusSGD(bann, g, data, labels, lr=lr, tracking=True, **kw)
