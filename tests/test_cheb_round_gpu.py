"""GPU parity of the Chebyshev round (dl_cheb_round) with its definition: the oracle's mix
(cref.mix_round, G = None) combined by the rule of include/dlamd.h, y = float32(a) * ACC +
float32(b) * Z in numpy -- three consecutive rounds with distinct (a, b), y being z, x or
neither.  The rounds are bit-exact, deviations within 1e-5 relative; the accelerated loop
(GossipEngine.mix_chebyshev, Mixer.mix_chebyshev) stops at the numpy restatement's round with
its bits."""
import functools
import logging

import numpy as np
import pytest
import torch

import cheb_oracle as O
from oracle import cref
from test_mix_gpu import DEV_RTOL, bits, check_dev, dev_floor, graph_csr
from test_sgd_round_gpu import FAMILIES, SHAPES, dev_t, family_params, problem, same

pytestmark = pytest.mark.gpu

ROUNDS = 3
COEFS = [(1.5, -0.5), (1.2371, -0.2371), (0.75, 0.5)]   # distinct; a + b need not be 1
MODES = ["y=z", "y=x", "apart"]


def E():
    from distributed_learning_amd import engine
    return engine


def operands(n, P, deg, weights="random"):
    """(csr, X0, Z0): test_sgd_round_gpu's problem, its first gradient matrix as z -- a random
    matrix unrelated to x."""
    csr, X0, Gs = problem(n, P, deg, weights)
    return csr, X0, Gs[0]


@functools.lru_cache(maxsize=None)
def oracle(n, P, deg, mode, weights="random", rounds=ROUNDS):
    """[y after round 1..rounds].  y == z and y apart ping-pong (the next round mixes y against
    the x it came from); y == x overwrites x and keeps z."""
    csr, X, Z = operands(n, P, deg, weights)
    out = []
    for a, b in COEFS[:rounds]:
        Y = O.cheb_step(cref.mix_round(X, csr.rowptr, csr.col, csr.w), Z, a, b)
        X, Z = (Y, Z) if mode == "y=x" else (Y, X)
        out.append(Y)
    return out


def run_rounds(cuda, csr, X0, Z0, mode, ld=None, sentinel=None, dev=False, rounds=ROUNDS,
               two_launch=False):
    """``rounds`` rounds on row-major operands (ld: row stride, the padding filled with
    ``sentinel``).  Returns ([y per round], last (dev_sq, dev_max, mean), the padded buffers).
    two_launch: dl_mix_round into a scratch, then dl_axpby (y == z only)."""
    eng = E()
    n, P = X0.shape
    ld = ld or P
    W = eng.DeviceCsr(csr, cuda)

    def padded(a=None):
        t = torch.full((n, ld), sentinel if sentinel is not None else 0.0, device=cuda)
        t[:, :P] = dev_t(a, cuda) if a is not None else 0.0
        return t
    Xb, Zb, Yb = padded(X0), padded(Z0), padded()
    dsq = torch.empty(n, device=cuda) if dev else None
    dmax = torch.empty(1, device=cuda) if dev else None
    mean = torch.empty(P, device=cuda) if dev else None
    if not two_launch:
        plan = eng.cheb_round_plan(W, Xb[:, :P], Zb[:, :P], Zb[:, :P], deviation=dev)
        assert plan is not None and plan["path"] == 1
    out = []
    for a, b in COEFS[:rounds]:
        X, Z = Xb[:, :P], Zb[:, :P]
        Y = {"y=z": Z, "y=x": X, "apart": Yb[:, :P]}[mode]
        if two_launch:
            S = torch.empty(n, P, device=cuda)
            eng.mix_round(W, X, S)
            eng.axpby(S, Z, a, b, out=Y)
        else:
            assert eng.cheb_round(W, X, Y, Z, a, b, dev_sq=dsq, dev_max=dmax, mean=mean) is True
        if mode == "y=z":
            Xb, Zb = Zb, Xb
        elif mode == "apart":
            Xb, Zb, Yb = Yb, Xb, Zb
        torch.cuda.synchronize()
        out.append(Xb[:, :P].cpu().numpy())
    devs = (dsq.cpu().numpy(), float(dmax.item()), mean.cpu().numpy()) if dev else None
    return out, devs, (Xb, Zb, Yb)


@pytest.mark.parametrize("n,P,deg", SHAPES)
def test_bits_match_the_rule_and_the_two_launches(cuda, n, P, deg):
    csr, X0, Z0 = operands(n, P, deg)
    for mode in MODES:
        want = oracle(n, P, deg, mode)
        got, _, _ = run_rounds(cuda, csr, X0, Z0, mode)
        for i in range(ROUNDS):
            same(got[i], want[i], f"y, round {i + 1}, {mode}")
    two, _, _ = run_rounds(cuda, csr, X0, Z0, "y=z", two_launch=True)
    same(two[-1], oracle(n, P, deg, "y=z")[-1], "y of dl_mix_round + dl_axpby")


def test_workgroups_walk_three_tiles(cuda):
    """n_tiles >= 3 x grid (both from dl_cheb_round_plan): the prefetch loop runs more than once
    per workgroup; with a ragged tail tile behind the full ones."""
    eng = E()
    n, deg = 64, 4
    csr = graph_csr(n, deg, seed=5)
    W = eng.DeviceCsr(csr, cuda)

    def plan(P):
        t = [torch.empty(n, P, device=cuda) for _ in range(2)]
        return eng.cheb_round_plan(W, t[0], t[1], t[1])
    p0 = plan(1 << 20)
    P = 3 * p0["grid"] * p0["tile_cols"] + 4     # (rows stay 16-byte aligned: the float4 kernel)
    assert n * P * 4 <= 256 << 20
    p = plan(P)
    assert p is not None and p["path"] == 1 and p["n_tiles"] >= 3 * p["grid"], p
    assert P % p["tile_cols"] != 0
    rng = np.random.default_rng(1)
    X0 = rng.standard_normal((n, P), dtype=np.float32)
    Z0 = rng.standard_normal((n, P), dtype=np.float32)
    for mode in ("y=z", "y=x"):
        X, Z = X0, Z0
        for a, b in COEFS[:2]:
            Y = O.cheb_step(cref.mix_round(X, csr.rowptr, csr.col, csr.w), Z, a, b)
            X, Z = (Y, Z) if mode == "y=x" else (Y, X)
        got, _, _ = run_rounds(cuda, csr, X0, Z0, mode, rounds=2)
        same(got[-1], X, f"y ({mode})")


@pytest.mark.parametrize("n,P,deg,weights", [(256, 1030, 4, "regular"), (300, 777, 8, "random"),
                                             (1500, 64, 6, "random"), (64, 4096, 4, "regular"),
                                             (64, 4096, 4, "random"), (1024, 4100, 4, "random")])
def test_deviation(cuda, n, P, deg, weights):
    """dev_sq, dev_max and mean of y for a z unrelated to x: one pass for a doubly stochastic W
    (uniform weights on a regular graph), two passes otherwise."""
    csr, X0, Z0 = operands(n, P, deg, weights)
    assert bool(csr.doubly_stochastic) == (weights == "regular")
    want = oracle(n, P, deg, "y=z", weights)
    for mode in ("y=z", "apart"):
        got, (dsq, dmax, mean), _ = run_rounds(cuda, csr, X0, Z0, mode, dev=True)
        same(got[-1], want[-1], f"y ({mode})")
        check_dev(got[-1], dsq, dmax, mean)


@pytest.mark.parametrize("n,tiles,weights,dev", FAMILIES)
def test_kernel_families_without_another_case(cuda, n, tiles, weights, dev):
    """mix_cheb_tile_kernel's instantiation families that no shape above reaches: those of
    test_sgd_round_gpu.FAMILIES (the two rounds are shaped alike), full tiles and a 5-column tail
    at an aligned row stride; the larger tile counts make a workgroup walk to a second tile."""
    P, deg = family_params(tiles), 4
    csr, X0, Z0 = operands(n, P, deg, weights)
    want = oracle(n, P, deg, "y=z", weights)
    t = [torch.empty(n, P + 3, device=cuda)[:, :P] for _ in range(2)]
    plan = E().cheb_round_plan(E().DeviceCsr(csr, cuda), t[0], t[1], t[1], deviation=dev)
    assert plan["tile_cols"] == 128 and plan["n_tiles"] >= tiles, plan
    assert tiles == 3 or plan["grid"] < tiles, plan   # a workgroup walks more than one tile
    got, devs, bufs = run_rounds(cuda, csr, X0, Z0, "y=z", ld=P + 3, sentinel=-7.25, dev=dev)
    for i in range(ROUNDS):
        same(got[i], want[i], f"y, round {i + 1}")
    for t in bufs:
        assert torch.all(t[:, P:] == -7.25)
    if dev:
        check_dev(got[-1], *devs)


@pytest.mark.parametrize("mode", ["y=z", "apart"])
@pytest.mark.parametrize("n,P,deg", [(33, 129, 4), (64, 4096, 4), (300, 777, 8)])
def test_padding_columns_are_never_written(cuda, n, P, deg, mode):
    """Row-major with ld = P + 4 (129 + 4: rows not 16-byte aligned, the guarded kernel; 4096 + 4:
    the float4 kernel): sentinels in the padding of every operand survive."""
    csr, X0, Z0 = operands(n, P, deg)
    got, _, bufs = run_rounds(cuda, csr, X0, Z0, mode, ld=P + 4, sentinel=-7.25)
    same(got[-1], oracle(n, P, deg, mode)[-1], "y")
    for t in bufs:
        assert torch.all(t[:, P:] == -7.25)


def engine_rounds(g, Z0, deviation=True):
    """ROUNDS x round_cheb on engine g (X loaded), its previous iterate set to Z0."""
    g.Y = g.layout_like(dev_t(Z0, g.device))
    for a, b in COEFS:
        g.round_cheb(a, b, deviation=deviation)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,P,deg", [(64, 4096, 4), (300, 777, 8)])
def test_tiled_engine_round_cheb(cuda, n, P, deg):
    """GossipEngine(layout="tiled").round_cheb: rows() is the row-major result's bits."""
    eng = E()
    csr, X0, Z0 = operands(n, P, deg)
    want = oracle(n, P, deg, "y=z")
    g = eng.GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda), layout="tiled")
    assert g.layout == "tiled" and g.order is None
    g.Y = g.layout_like(dev_t(Z0, cuda))
    assert eng.cheb_round_plan(g.W, g.X, g.Y, g.Y, tiled=(P, g.T), deviation=True) is not None
    engine_rounds(g, Z0)
    same(g.rows().cpu().numpy(), want[-1], "rows()")
    np.testing.assert_allclose(np.sqrt(g.dev_sq.cpu().numpy()),
                               np.sqrt(cref.deviation_sq(want[-1])), rtol=DEV_RTOL)


def test_fallback_when_the_plan_is_not_path_1(cuda, monkeypatch):
    monkeypatch.setenv("DLAMD_FORCE_GATHER", "1")
    eng = E()
    n, P, deg = 64, 1000, 4
    csr, X0, Z0 = operands(n, P, deg)
    g = eng.GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda), layout="rows")
    assert g.plan()["path"] == 2 and g.layout == "rows"
    g.Y = g.layout_like(dev_t(Z0, cuda))
    assert eng.cheb_round_plan(g.W, g.X, g.Y, g.Y) is None               # UNSUPPORTED
    assert eng.cheb_round(g.W, g.X, g.Y, g.Y, 1.5, -0.5) is False
    engine_rounds(g, Z0)
    want = oracle(n, P, deg, "y=z")
    same(g.rows().cpu().numpy(), want[-1], "rows()")
    np.testing.assert_allclose(np.sqrt(g.dev_sq.cpu().numpy()),
                               np.sqrt(cref.deviation_sq(want[-1])), rtol=DEV_RTOL)


def test_fallback_in_the_tiled_layout(cuda, monkeypatch):
    """Plan path 4 (the register-CSR kernel) keeps the tiled layout: the plain round mixes into
    the scratch, dl_axpby runs over the resident buffers as one row each."""
    monkeypatch.setenv("DLAMD_FORCE_REG", "1")
    eng = E()
    n, P = 1500, 64
    csr, X0, Z0 = operands(n, P, 4, "regular")
    g = eng.GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda))
    assert g.plan()["path"] == 4 and g.layout == "tiled"
    g.Y = g.layout_like(dev_t(Z0, cuda))
    assert eng.cheb_round_plan(g.W, g.X, g.Y, g.Y, tiled=(P, g.T)) is None
    assert eng.cheb_round(g.W, g.X, g.Y, g.Y, 1.5, -0.5, tiled=(P, g.T)) is False
    engine_rounds(g, Z0, deviation=False)
    same(g.rows().cpu().numpy(), oracle(n, P, 4, "y=z", "regular")[-1], "rows()")


def test_captured_rounds_replay_the_eager_bits(cuda):
    """One graph per ping-pong parity with a fixed (a, b); replayed alternately, four replays give
    the bits and the deviation of four eager rounds."""
    eng = E()
    n, P, deg = 64, 4096, 4
    a, b = 1.2371, -0.2371
    csr, X0, Z0 = operands(n, P, deg)

    def fresh():
        g = eng.GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda))
        g.Y = g.layout_like(dev_t(Z0, cuda))
        g.reserve_workspace(deviation=True)
        return g
    e = fresh()
    for _ in range(4):
        e.round_cheb(a, b, deviation=True)
    torch.cuda.synchronize()
    g = fresh()
    torch.cuda.synchronize()
    graphs = []
    for _ in range(2):
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            g.round_cheb(a, b, deviation=True)
        graphs.append(cg)
    torch.cuda.synchronize()
    same(g.rows().cpu().numpy(), X0, "capture ran nothing")
    for i in range(4):
        graphs[i % 2].replay()
    torch.cuda.synchronize()
    assert torch.equal(g.X, e.X) and torch.equal(g.Y, e.Y)
    assert torch.equal(g.dev_sq, e.dev_sq) and torch.equal(g.dev_max, e.dev_max)
    X, Z = X0, Z0
    for _ in range(4):
        X, Z = O.cheb_step(cref.mix_round(X, csr.rowptr, csr.col, csr.w), Z, a, b), X
    same(g.rows().cpu().numpy(), X, "rows() after four replays")


# ---- the loop ----

@functools.lru_cache(maxsize=None)
def loop_oracle(n, P):
    """(csr, gamma, X0, [(X, dev)] of the Chebyshev rounds, k*, eps, plain rounds to eps)."""
    csr, gamma, X0 = O.problem(n, P)
    seq = O.cheb_rounds(csr, X0, gamma, 80)
    devs = [d for _, d in seq]
    kstar, eps = O.margin_eps(devs, below=1e-2)
    plain = O.rounds_until([d for _, d in O.plain_rounds(csr, X0, 1200)], eps)
    return csr, gamma, X0, seq, kstar, eps, plain


def check_margins(seq, kstar, eps):
    """On the CPU: every deviation before round k* exceeds 1.01 eps and d_k* < 0.99 eps, so a
    device deviation within 1e-5 relative cannot move the count."""
    devs = [d for _, d in seq]
    assert all(d > 1.01 * eps for d in devs[:kstar - 1]) and devs[kstar - 1] < 0.99 * eps
    assert O.rounds_until(devs, eps) == kstar


@pytest.mark.parametrize("layout", ["auto", "rows"])
@pytest.mark.parametrize("n,P", [(64, 256), (33, 129)])
def test_engine_mix_chebyshev(cuda, n, P, layout):
    eng = E()
    csr, gamma, X0, seq, kstar, eps, plain = loop_oracle(n, P)
    check_margins(seq, kstar, eps)
    print(f"n={n} P={P} gamma={gamma:.6f} eps={eps:.4e}: Chebyshev {kstar} rounds, plain {plain}")
    g = eng.GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda), layout=layout)
    seen = []
    done = g.mix_chebyshev(gamma, times=1, eps=eps, on_deviation=seen.append)
    assert done == kstar and len(seen) == kstar
    same(g.rows().cpu().numpy(), seq[kstar - 1][0], "final iterate")
    # every evaluated deviation against the fp64 one: check_dev's bar
    floor = dev_floor(X0.astype(np.float64).mean(axis=0), P)
    np.testing.assert_allclose(seen, [d for _, d in seq[:kstar]], rtol=DEV_RTOL, atol=floor)
    assert plain is not None and 4 * done <= plain
    # times is a floor on the rounds: the rule holds first at round k*, so times = k* + 3 stops
    # at the first later round below eps
    later = O.rounds_until([d for _, d in seq], eps, times=kstar + 3)
    assert later is not None
    g.load_rows(dev_t(X0, cuda))
    d = [d for _, d in seq]
    if all(abs(x - eps) > 0.01 * eps for x in d[kstar:later]):
        assert g.mix_chebyshev(gamma, times=kstar + 3, eps=eps) == later
        same(g.rows().cpu().numpy(), seq[later - 1][0], "iterate at the later stop")
        g.load_rows(dev_t(X0, cuda))
    # eps = None: exactly ceil(times) rounds
    assert g.mix_chebyshev(gamma, times=4.5) == 5
    same(g.rows().cpu().numpy(), seq[4][0], "iterate after 5 rounds")
    with pytest.raises(ValueError):
        g.mix_chebyshev(1.0)


@pytest.mark.parametrize("n,P,shape", [(64, 256, (16, 15)), (33, 129, (1, 128))])
def test_mixer_mix_chebyshev(cuda, n, P, shape):
    """Mixer.mix_chebyshev flattens, runs the loop, writes the models back and logs as mix does;
    Mixer.mix on the same object still runs the plain rounds."""
    from distributed_learning_amd.utils.consensus_simple.mixer import Mixer
    csr, gamma, X0, seq, kstar, eps, plain = loop_oracle(n, P)
    check_margins(seq, kstar, eps)
    models = []
    for a in range(n):
        m = torch.nn.Linear(shape[1], shape[0]).to(cuda)
        with torch.no_grad():
            m.weight.copy_(dev_t(X0[a, :shape[0] * shape[1]], cuda).view(shape))
            m.bias.copy_(dev_t(X0[a, shape[0] * shape[1]:], cuda))
        models.append(m)
    topology = {a: {int(c): float(w) for c, w in zip(csr.col[csr.rowptr[a]:csr.rowptr[a + 1]],
                                                       csr.w[csr.rowptr[a]:csr.rowptr[a + 1]])}
                for a in range(n)}
    lines = []

    class Keep(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())
    logger = logging.getLogger(f"cheb_mixer_{n}")
    logger.setLevel(logging.DEBUG)
    logger.propagate = False
    logger.handlers = [Keep()]
    mixer = Mixer(models, topology, logger, device=cuda)

    def flat():
        return torch.stack([torch.cat([p.data.view(-1) for p in m.parameters()])
                            for m in models]).cpu().numpy()
    same(flat(), X0, "models hold X0")
    done = mixer.mix_chebyshev(gamma, times=1, eps=eps)
    assert done == kstar and 4 * done <= plain
    same(flat(), seq[kstar - 1][0], "models after mix_chebyshev")
    assert lines[0] == 'Mixer start with times= {}, eps= {}'.format(1, eps)
    assert lines[-1] == 'Mixer finished with {} times'.format(kstar)
    assert [ln.startswith('Mixer calculate max deviation= ') for ln in lines[1:-1]] == \
        [True] * kstar
    # mix itself is untouched: two plain rounds from here
    X = seq[kstar - 1][0]
    for _ in range(2):
        X = cref.mix_round(X, csr.rowptr, csr.col, csr.w)
    assert mixer.mix(times=2) == 2
    same(flat(), X, "models after mix")
    with pytest.raises(ValueError):
        mixer.mix_chebyshev(0.0)
