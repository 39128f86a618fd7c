"""GPU parity of the fused Adam round (dl_adam_round), the Adam step (dl_adam_step) and the device
step count (dl_adam_tick) with their definition (adam_oracle: one fp32 numpy operation per line
of include/dlamd.h, the recurrence in Python floats, then the oracle's fold) -- three consecutive
steps with a distinct gradient each, so that both moments and the bias corrections are carried,
x' in place or apart, the coefficients by value or from the device.  X, M and V are bit-exact,
deviations within 1e-5 relative; the composed two-launch form gives the same bits."""
import functools

import numpy as np
import pytest
import torch

import adam_oracle as O
from oracle import cref
from test_mix_gpu import DEV_RTOL, bits, check_dev, graph_csr
from test_sgd_round_gpu import FAMILIES, SHAPES, dev_t, family_params, problem, same

pytestmark = pytest.mark.gpu

LR = 0.01
STEPS = 3
OPTS = {"plain": dict(weight_decay=0.0, decoupled=False),
        "l2": dict(weight_decay=5e-4, decoupled=False),
        "decoupled": dict(weight_decay=1e-2, decoupled=True)}


def E():
    from distributed_learning_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def oracle(n, P, deg, opt, weights="random"):
    """[(X, M, V) after step 1..STEPS] from m = v = 0: the same for every aliasing mode."""
    csr, X0, Gs = problem(n, P, deg, weights)
    return O.adam_rounds(csr, X0, Gs, LR, **OPTS[opt])


def run_rounds(cuda, csr, X0, Gs, opt, in_place=False, ld=None, sentinel=None, dev=False,
               composed=False, device_coef=False, M0=None, V0=None):
    """len(Gs) rounds on row-major operands (ld: row stride, the padding filled with
    ``sentinel``) from t = 0.  Returns ([(X, M, V) per round], last (dev_sq, dev_max, mean),
    every padded buffer).  composed: dl_adam_step into S, dl_mix_round of S.  device_coef: the
    coefficients from an AdamState ticked on the device, else by value from its host mirror."""
    eng = E()
    n, P = X0.shape
    ld = ld or P
    W = eng.DeviceCsr(csr, cuda)

    def padded(a=None):
        t = torch.full((n, ld), sentinel if sentinel is not None else 0.0, device=cuda)
        t[:, :P] = dev_t(a, cuda) if a is not None else 0.0
        return t
    Xb, Yb, Mb, Vb, Sb = padded(X0), padded(), padded(M0), padded(V0), padded()
    Gb = [padded(G) for G in Gs]
    dsq = torch.empty(n, device=cuda) if dev else None
    dmax = torch.empty(1, device=cuda) if dev else None
    mean = torch.empty(P, device=cuda) if dev else None
    v = lambda t: t[:, :P]   # noqa: E731
    if not composed:
        plan = eng.adam_round_plan(W, v(Xb), v(Yb), v(Gb[0]), v(Mb), v(Vb), deviation=dev)
        assert plan is not None and plan["path"] == 1
    st = eng.AdamState(LR, device=cuda if device_coef else None)
    out = []
    for i in range(len(Gs)):
        st.tick()
        kw = dict(lr=LR, coef=st.coef, **opt) if device_coef else \
            dict(lr=LR, step_size=st.step_size, bias2_sqrt=st.bias2_sqrt, **opt)
        X, G, M, V = v(Xb), v(Gb[i]), v(Mb), v(Vb)
        Y = X if in_place else v(Yb)
        if composed:
            eng.adam_step(X, G, M, V, out=v(Sb), **kw)
            eng.mix_round(W, v(Sb), v(Yb), dev_sq=dsq, dev_max=dmax, mean=mean)
            Y = v(Yb)
        else:
            assert eng.adam_round(W, X, Y, G, M, V, dev_sq=dsq, dev_max=dmax, mean=mean,
                                  **kw) is True
        if Y is not X:
            Xb, Yb = Yb, Xb
        torch.cuda.synchronize()
        out.append((v(Xb).cpu().numpy(), M.cpu().numpy(), V.cpu().numpy()))
    devs = (dsq.cpu().numpy(), float(dmax.item()), mean.cpu().numpy()) if dev else None
    return out, devs, [Xb, Yb, Mb, Vb] + Gb


def check_rounds(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip("MVX", (g[1], g[2], g[0]), (w[1], w[2], w[0])):
            same(a, b, f"{name}, round {i + 1}, {what}")


@pytest.mark.parametrize("opt", list(OPTS))
@pytest.mark.parametrize("n,P,deg", SHAPES)
def test_bits_match_the_oracle_and_the_composed_form(cuda, n, P, deg, opt):
    csr, X0, Gs = problem(n, P, deg)
    want = oracle(n, P, deg, opt)
    got, _, _ = run_rounds(cuda, csr, X0, Gs, OPTS[opt])
    check_rounds(got, want, "x' apart, coefficients by value")
    got, _, _ = run_rounds(cuda, csr, X0, Gs, OPTS[opt], in_place=True, device_coef=True)
    check_rounds(got, want, "x' = x, coefficients from the device")
    comp, _, _ = run_rounds(cuda, csr, X0, Gs, OPTS[opt], composed=True)
    check_rounds(comp, want, "dl_adam_step + dl_mix_round")


@pytest.mark.parametrize("n,tiles,weights,dev", FAMILIES)
def test_kernel_families(cuda, n, tiles, weights, dev):
    """mix_adam_tile_kernel's instantiation families (those of test_sgd_round_gpu.FAMILIES: the
    rounds are shaped alike): 2 / 4 / 8 rows per thread -- all four streams prefetched, x and g,
    x alone -- five-weight and CSR rows, the mean from the staged s and the two-pass form, the
    tile walk, and a ragged 5-column tail on the guarded kernel, at ld = P + 3 with a sentinel in
    the padding of x, y, g, m and v."""
    P, deg = family_params(tiles), 4
    csr, X0, Gs = problem(n, P, deg, weights)
    want = oracle(n, P, deg, "l2", weights)
    t = [torch.empty(n, P + 3, device=cuda)[:, :P] for _ in range(5)]
    plan = E().adam_round_plan(E().DeviceCsr(csr, cuda), *t, deviation=dev)
    assert plan["tile_cols"] == 128 and plan["n_tiles"] >= tiles, plan
    assert tiles == 3 or plan["grid"] < tiles, plan   # a workgroup walks more than one tile
    got, devs, bufs = run_rounds(cuda, csr, X0, Gs, OPTS["l2"], ld=P + 3, sentinel=-7.25, dev=dev,
                                 device_coef=True)
    check_rounds(got, want, "families")
    for b in bufs:
        assert torch.all(b[:, P:] == -7.25)
    if dev:
        check_dev(got[-1][0], *devs)


def test_workgroups_walk_three_tiles(cuda):
    """n_tiles >= 3 x grid (both from dl_adam_round_plan): the cross-tile prefetch and the
    in-tile loads run more than once per workgroup; with a ragged tail tile behind the full
    ones."""
    eng = E()
    n, deg = 64, 4
    csr = graph_csr(n, deg, seed=5)
    W = eng.DeviceCsr(csr, cuda)

    def plan(P):
        t = [torch.empty(n, P, device=cuda) for _ in range(5)]
        return eng.adam_round_plan(W, *t)
    p0 = plan(1 << 20)
    P = 3 * p0["grid"] * p0["tile_cols"] + 4     # (rows stay 16-byte aligned: the float4 kernel)
    assert n * P * 4 <= 256 << 20
    p = plan(P)
    assert p is not None and p["path"] == 1 and p["n_tiles"] >= 3 * p["grid"], p
    assert P % p["tile_cols"] != 0
    rng = np.random.default_rng(1)
    X0, G1, G2 = (rng.standard_normal((n, P), dtype=np.float32) for _ in range(3))
    want = O.adam_rounds(csr, X0, [G1, G2], LR, **OPTS["decoupled"])
    for in_place in (False, True):
        got, _, _ = run_rounds(cuda, csr, X0, [G1, G2], OPTS["decoupled"], in_place=in_place)
        check_rounds(got[-1:], want[-1:], f"in_place={in_place}")


@pytest.mark.parametrize("n,P,deg,weights", [(256, 1030, 4, "regular"), (300, 777, 8, "random"),
                                             (1500, 64, 6, "random"), (64, 4096, 4, "regular"),
                                             (64, 4096, 4, "random"), (1024, 4100, 4, "random")])
def test_deviation(cuda, n, P, deg, weights):
    """dev_sq, dev_max and mean of x': one pass for a doubly stochastic W (uniform weights on a
    regular graph), two passes otherwise."""
    csr, X0, Gs = problem(n, P, deg, weights)
    assert bool(csr.doubly_stochastic) == (weights == "regular")
    want = oracle(n, P, deg, "plain", weights)
    for in_place in (False, True):
        got, (dsq, dmax, mean), _ = run_rounds(cuda, csr, X0, Gs, OPTS["plain"],
                                               in_place=in_place, dev=True)
        check_rounds(got[-1:], want[-1:], f"in_place={in_place}")
        check_dev(got[-1][0], dsq, dmax, mean)


@pytest.mark.parametrize("in_place", [False, True])
def test_unaligned_rows_take_the_guarded_kernel(cuda, in_place):
    """33 x 129 at ld = P + 4 = 133: rows are not 16-byte aligned, so every tile runs the guarded
    kernel; sentinels in the padding of every operand survive."""
    n, P, deg = 33, 129, 4
    csr, X0, Gs = problem(n, P, deg)
    got, devs, bufs = run_rounds(cuda, csr, X0, Gs, OPTS["l2"], in_place=in_place, ld=P + 4,
                                 sentinel=-7.25, dev=True)
    check_rounds(got, oracle(n, P, deg, "l2"), f"in_place={in_place}")
    check_dev(got[-1][0], *devs)
    for b in bufs:
        assert torch.all(b[:, P:] == -7.25)


def same_with_nans(got, want, what):
    """NaN in the same places, the same bits everywhere else."""
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ ({gn.sum()} against {wn.sum()})"
    assert np.array_equal(bits(got)[~wn], bits(want)[~wn]), \
        f"{what}: {np.count_nonzero(bits(got)[~wn] != bits(want)[~wn])} elements differ"


@pytest.mark.parametrize("weights", ["regular", "random"])
def test_special_values(cuda, weights):
    """64 x 260 (two full 128-column tiles and a guarded 4-column tail): a first step with g = 0;
    gradients whose squares are subnormal or zero; one NaN and one +Inf gradient."""
    n, P, deg = 64, 260, 4
    csr, X0, _ = problem(n, P, deg, weights)
    rng = np.random.default_rng(64)
    # g = 0 from m = v = 0: v' = 0, den = eps, s = x, so the round is the plain mix of x
    Z = np.zeros_like(X0)
    got, _, _ = run_rounds(cuda, csr, X0, [Z], OPTS["plain"])
    with np.errstate(all="ignore"):
        same(got[0][0], cref.mix_round(np.array(X0), csr.rowptr, csr.col, csr.w), "x' with g = 0")
    assert not got[0][1].any() and not got[0][2].any()
    same(got[0][0], O.adam_rounds(csr, X0, [Z], LR)[0][0], "x' with g = 0 (oracle)")
    # |g| from 1e-26 to 1e-17: (omb2 g) g = 1e-3 g^2 is zero, subnormal or barely normal
    tiny = (10.0 ** rng.uniform(-26, -17, (n, P)) * rng.choice([-1.0, 1.0], (n, P)))
    tiny = tiny.astype(np.float32)
    want = O.adam_rounds(csr, X0, [tiny, tiny], LR)
    v1 = want[0][2]
    sub = (v1 > 0) & (v1 < np.finfo(np.float32).tiny)
    assert sub.any() and (v1 == 0).any() and (v1 >= np.finfo(np.float32).tiny).any()
    for kw in (dict(), dict(in_place=True, device_coef=True), dict(composed=True)):
        got, _, _ = run_rounds(cuda, csr, X0, [tiny, tiny], OPTS["plain"], **kw)
        check_rounds(got, want, f"tiny gradients {kw}")
    # one NaN and one +Inf in g: that element of m' and v', and the y of the rows that fold it
    G = rng.standard_normal((n, P), dtype=np.float32)
    (ra, ca), (rb, cb) = (5, 130), (40, 258)      # a full tile and the guarded tail
    G[ra, ca], G[rb, cb] = np.nan, np.inf
    M0 = rng.standard_normal((n, P), dtype=np.float32) * 0.1
    V0 = rng.random((n, P), dtype=np.float32) * 0.1
    want = O.adam_rounds(csr, X0, [G], LR, M=M0, V=V0)
    for kw in (dict(), dict(in_place=True), dict(composed=True)):
        got, _, _ = run_rounds(cuda, csr, X0, [G], OPTS["plain"], M0=M0, V0=V0, **kw)
        for name, a, b in zip("XMV", got[0], want[0]):
            same_with_nans(a, b, f"{name} with a NaN and an Inf gradient {kw}")
        x, m, v = got[0]
        assert np.isnan(m[ra, ca]) and np.isnan(v[ra, ca]) and np.isnan(m).sum() == 1
        assert np.isposinf(m[rb, cb]) and np.isposinf(v[rb, cb])
        assert np.isfinite(m).sum() == m.size - 2 and np.isfinite(v).sum() == v.size - 2
        rp, cl = np.asarray(csr.rowptr), np.asarray(csr.col)
        for r, c in ((ra, ca), (rb, cb)):
            folds = np.array([r in cl[rp[a]:rp[a + 1]] for a in range(n)])
            assert np.array_equal(np.isnan(x[:, c]), folds)
        assert np.isnan(x).sum() == np.isnan(x[:, ca]).sum() + np.isnan(x[:, cb]).sum()


def test_tick_follows_the_python_recurrence(cuda):
    """The state and both coefficients after 1, 2, 10 and 1000 ticks are the Python recurrence's
    bit for bit; an lr written into the state changes the next step_size alone."""
    eng = E()
    lr, betas = 3e-3, (0.9, 0.999)
    st, c = eng.AdamState(lr, betas, device=cuda), O.Coefs(lr, betas)
    assert np.array_equal(st.state.cpu().numpy().view(np.uint64), c.state().view(np.uint64))
    for t in range(1, 1001):
        st.tick()
        c.tick()
        if t in (1, 2, 10, 1000):
            got = st.state.cpu().numpy()
            assert np.array_equal(got.view(np.uint64), c.state().view(np.uint64)), (t, got)
            coef = st.coef.cpu().numpy()
            assert coef.tobytes() == np.array([c.step_size, c.bias2_sqrt]).tobytes()
            assert (st.t, st.step_size, st.bias2_sqrt) == (t, c.step_size, c.bias2_sqrt)
    st.set_lr(7e-4)
    c.lr = 7e-4
    st.tick()
    c.tick()
    assert np.array_equal(st.state.cpu().numpy().view(np.uint64), c.state().view(np.uint64))
    assert st.coef.cpu().numpy()[0] == np.float32(7e-4 / (1.0 - c.b1t)) == st.step_size
    st.reset()
    assert np.array_equal(st.state.cpu().numpy().view(np.uint64),
                          O.Coefs(7e-4, betas).state().view(np.uint64))


def agent_rows(g, A):
    """A resident matrix of engine g as row-major rows in agent order."""
    R = E().from_tiled(A, g.P) if g.layout == "tiled" else A
    if g.order is not None:
        out = torch.empty_like(R)
        out[g.order] = R
        R = out
    return R.cpu().numpy()


@pytest.mark.parametrize("knob", [None, "DLAMD_FORCE_GATHER", "DLAMD_FORCE_REG"])
@pytest.mark.parametrize("n,P,deg", [(64, 4096, 4), (300, 777, 8)])
def test_tiled_engine_round_adam(cuda, monkeypatch, n, P, deg, knob):
    """GossipEngine.round_adam in the column-tiled layout: rows(), M and V converted back are the
    row-major result's bits.  With the gather path forced (row-major: plan path 2) and with the
    register-CSR path forced (column-tiled, plan path 5 under a row order) the fused round is
    refused and the composed dl_adam_step + round() runs: the same bits."""
    if knob:
        monkeypatch.setenv(knob, "1")
    eng = E()
    csr, X0, Gs = problem(n, P, deg)
    want = oracle(n, P, deg, "l2")
    g = eng.GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda),
                         layout="rows" if knob == "DLAMD_FORCE_GATHER" else "tiled")
    g.reset_adam(LR)
    tiled = (P, g.T) if g.layout == "tiled" else None
    G0 = g.layout_like(dev_t(Gs[0], cuda))
    plan = eng.adam_round_plan(g.W, g.X, g.Y, G0, g.M, g.V, tiled=tiled, deviation=True)
    if knob is None:
        assert g.layout == "tiled" and g.order is None and plan is not None
    else:
        assert g.plan()["path"] == (2 if knob == "DLAMD_FORCE_GATHER" else 5) and plan is None
        assert eng.adam_round(g.W, g.X, g.Y, G0, g.M, g.V, lr=LR, coef=g.adam.coef,
                              tiled=tiled) is False
    for G in Gs:     # (fused where it plans, whatever the engine's default)
        g.round_adam(g.layout_like(dev_t(G, cuda)), LR, deviation=True, fused=True, **OPTS["l2"])
    torch.cuda.synchronize()
    assert g.adam.t == STEPS
    same(g.rows().cpu().numpy(), want[-1][0], "rows()")
    same(agent_rows(g, g.M), want[-1][1], "M")
    same(agent_rows(g, g.V), want[-1][2], "V")
    np.testing.assert_allclose(np.sqrt(g.agent_dev_sq().cpu().numpy()),
                               np.sqrt(cref.deviation_sq(want[-1][0])), rtol=DEV_RTOL)
    g.reset_adam()
    assert g.adam.t == 0 and not g.M.any() and not g.V.any()
    assert g.adam.state.cpu().numpy()[0] == 0.0


def test_captured_rounds_replay_the_eager_bits(cuda):
    """The tick and the round in one graph per parity; replayed alternately, four replays give the
    bits and the deviation of four eager rounds -- every replay is the next Adam step."""
    eng = E()
    n, P, deg = 64, 4096, 4
    csr, X0, Gs = problem(n, P, deg)

    def fresh():
        g = eng.GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda))
        g.reset_adam(LR)
        g.reserve_workspace(deviation=True)
        return g, [g.layout_like(dev_t(Gs[0], cuda)), g.layout_like(dev_t(Gs[1], cuda))]
    e, eb = fresh()
    for i in range(4):
        e.round_adam(eb[i % 2], LR, deviation=True, fused=True, **OPTS["decoupled"])
    torch.cuda.synchronize()
    g, gb = fresh()
    torch.cuda.synchronize()
    graphs = []
    for i in range(2):
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            g.round_adam(gb[i], LR, deviation=True, fused=True, **OPTS["decoupled"])
        graphs.append(cg)
    torch.cuda.synchronize()
    same(g.rows().cpu().numpy(), X0, "capture ran nothing (X)")
    assert not g.M.any() and not g.V.any() and g.adam.state.cpu().numpy()[0] == 0.0
    for i in range(4):
        graphs[i % 2].replay()
    torch.cuda.synchronize()
    assert torch.equal(g.X, e.X) and torch.equal(g.M, e.M) and torch.equal(g.V, e.V)
    assert torch.equal(g.dev_sq, e.dev_sq) and torch.equal(g.dev_max, e.dev_max)
    assert torch.equal(g.adam.state, e.adam.state) and g.adam.state.cpu().numpy()[0] == 4.0
    want = O.adam_rounds(csr, X0, [Gs[0], Gs[1], Gs[0], Gs[1]], LR, **OPTS["decoupled"])
    same(g.rows().cpu().numpy(), want[-1][0], "rows() after four replays")
    same(agent_rows(g, g.M), want[-1][1], "M after four replays")
    same(agent_rows(g, g.V), want[-1][2], "V after four replays")


def test_mlp_consensus_sgd_with_adam(cuda):
    """MLPConsensusSGD(optimizer="adam") with BatchedANN, 4 agents x 64 samples on a ring: three
    eager steps are a hand-composed loop of ann.gradients and engine.adam_round with the
    coefficients by value; then capture() and two replay()s equal two further eager steps of a
    twin, bit for bit."""
    from distributed_learning_amd.graph import Csr
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    from distributed_learning_amd.workloads import MLPConsensusSGD
    eng = E()
    n, b, lr, opt = 4, 64, 1e-2, dict(betas=(0.8, 0.99), eps=1e-6, weight_decay=5e-4)
    cl = np.concatenate([[a, (a + 1) % n, (a - 1) % n] for a in range(n)])
    csr = Csr(np.arange(0, 3 * n + 1, 3), cl, np.full(cl.size, 1.0 / 3))
    gen = torch.Generator(device=cuda).manual_seed(7)
    bann = BatchedANN(n, b, 64, 32, 10, device=cuda)
    X0 = 0.1 * torch.randn(n, bann.P, device=cuda, generator=gen)
    data = torch.randn(n, b, 64, device=cuda, generator=gen)
    labels = torch.randint(0, 10, (n, b), device=cuda, generator=gen, dtype=torch.int32)

    def trainer():
        g = eng.GossipEngine(csr, bann.P, device=cuda, X=X0)
        return g, MLPConsensusSGD(bann, g, data, labels, lr=lr, optimizer="adam", **opt)
    g, sgd = trainer()
    assert sgd.adam and torch.count_nonzero(g.M) == 0 and g.adam.t == 0
    for _ in range(3):
        sgd.step()
    # the same three steps by hand
    h = eng.GossipEngine(csr, bann.P, device=cuda, X=X0)
    assert h.layout == g.layout
    tiled = (h.P, h.T) if h.layout == "tiled" else None
    M, V, G = torch.zeros_like(h.X), torch.zeros_like(h.X), torch.zeros_like(h.X)
    st = eng.AdamState(lr, opt["betas"])
    for i in range(3):
        if tiled:
            bann.gradients(h.X, data, labels, G)
        else:
            bann.gradients(h.X[:, :bann.P], data, labels, G[:, :bann.P])
        st.tick()
        assert eng.adam_round(h.W, h.X, h.Y, G, M, V, lr=lr, step_size=st.step_size,
                              bias2_sqrt=st.bias2_sqrt, dev_sq=h.dev_sq, dev_max=h.dev_max,
                              workspace=h.ws, tiled=tiled, **opt) is True
        h.X, h.Y = h.Y, h.X
    torch.cuda.synchronize()
    assert torch.equal(g.X, h.X) and torch.equal(g.M, M) and torch.equal(g.V, V)
    assert torch.equal(g.dev_sq, h.dev_sq)
    assert not torch.equal(g.rows(), X0) and torch.count_nonzero(g.V) > 0
    # a twin runs five eager steps; this one three, then two replays
    t, twin = trainer()
    for _ in range(5):
        twin.step()
    sgd.capture()
    assert g.adam.t == 3 and sgd.steps_done == 3
    sgd.replay(2)
    torch.cuda.synchronize()
    assert sgd.steps_done == twin.steps_done == 5 and g.adam.t == t.adam.t == 5
    assert torch.equal(g.X, t.X) and torch.equal(g.M, t.M) and torch.equal(g.V, t.V)
    assert torch.equal(g.dev_sq, t.dev_sq) and torch.equal(g.adam.state, t.adam.state)
    assert g.adam.step_size == t.adam.step_size
    with pytest.raises(ValueError, match="exclusive"):
        MLPConsensusSGD(bann, g, data, labels, lr=lr, optimizer="adam", tracking=True)
    for kw in (dict(momentum=0.9), dict(nesterov=True), dict(emit="step"),
               dict(optimizer="rmsprop")):
        with pytest.raises(ValueError):
            MLPConsensusSGD(bann, g, data, labels, lr=lr, **{"optimizer": "adam", **kw})
