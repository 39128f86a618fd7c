"""GPU parity of the fused momentum-SGD round (dl_sgd_round) with its definition: the oracle's
torch.optim.SGD step (cref.sgd_step) followed by the oracle's mix (cref.mix_round, G = None),
three consecutive steps so that the momentum buffers are carried.  The mix and the buffers are
bit-exact, deviations within 1e-5 relative."""
import functools

import numpy as np
import pytest
import torch

from oracle import cref
from test_mix_gpu import DEV_RTOL, bits, check_dev, graph_csr

pytestmark = pytest.mark.gpu

LR = 0.05
STEPS = 3
# momentum, dampening, weight decay, nesterov
OPTS = [(0.9, 0.0, 5e-4, False), (0.9, 0.0, 0.0, True), (0.9, 0.1, 5e-4, False),
        (0.0, 0.0, 5e-4, False), (0.0, 0.0, 0.0, False)]
SHAPES = [(2, 7, 2), (33, 129, 4), (64, 4096, 4), (300, 777, 8), (1024, 4100, 4), (1500, 64, 6)]


def E():
    from distributed_learning_amd import engine
    return engine


def dev_t(a, cuda):
    """A device copy of a (read-only) numpy array."""
    return torch.from_numpy(np.array(a)).to(cuda)


def opt_kw(opt):
    return dict(momentum=opt[0], dampening=opt[1], weight_decay=opt[2], nesterov=opt[3])


def regular_csr(n):
    """A circulant graph of degree 4 with one uniform weight: symmetric, so doubly stochastic."""
    from distributed_learning_amd.graph import Csr
    cl = np.concatenate([[a, (a + 1) % n, (a - 1) % n, (a + 2) % n, (a - 2) % n]
                         for a in range(n)])
    csr = Csr(np.arange(0, 5 * n + 1, 5), cl, np.full(cl.size, 0.2))
    assert csr.doubly_stochastic and csr.uniform_row_nnz == 5
    return csr


@functools.lru_cache(maxsize=None)
def problem(n, P, deg, weights="random"):
    """(csr, X0, [G per step]) of a shape: built once, shared, never modified."""
    csr = regular_csr(n) if weights == "regular" else graph_csr(n, deg, seed=n + P)
    rng = np.random.default_rng(n * 7 + P)
    X0 = rng.standard_normal((n, P), dtype=np.float32)
    Gs = [rng.standard_normal((n, P), dtype=np.float32) for _ in range(STEPS)]
    for a in [X0] + Gs:
        a.setflags(write=False)
    return csr, X0, Gs


@functools.lru_cache(maxsize=None)
def oracle(n, P, deg, opt, weights="random"):
    """[(X, buf) after step 1, 2, 3]: cref.sgd_step then cref.mix_round(G=None)."""
    csr, X0, Gs = problem(n, P, deg, weights)
    X, buf, out = X0, (np.zeros_like(X0) if opt[0] != 0.0 else None), []
    for i, G in enumerate(Gs):
        S = cref.sgd_step(X, G, buf, lr=LR, first=i == 0, **opt_kw(opt))
        X = cref.mix_round(S, csr.rowptr, csr.col, csr.w)
        out.append((X, buf.copy() if buf is not None else None))
    return out


def fused_steps(cuda, csr, X0, Gs, opt, in_place=False, ld=None, sentinel=None, dev=False,
                buf_fill=0.0, steps=STEPS):
    """The fused round over ``steps`` steps on row-major operands (ld: row stride, the padding
    filled with ``sentinel``).  Returns ([(X, M) per step], last (dev_sq, dev_max, mean), the
    padded device buffers of the last step)."""
    eng = E()
    n, P = X0.shape
    ld = ld or P
    W = eng.DeviceCsr(csr, cuda)

    def padded(a=None, fill=0.0):
        t = torch.full((n, ld), sentinel if sentinel is not None else fill, device=cuda)
        if a is not None:
            t[:, :P] = dev_t(a, cuda)
        elif sentinel is not None:
            t[:, :P] = fill
        return t
    Xb, Yb = padded(X0), padded(fill=0.0)
    Mb = padded(fill=buf_fill) if opt[0] != 0.0 else None
    dsq = torch.empty(n, device=cuda) if dev else None
    dmax = torch.empty(1, device=cuda) if dev else None
    mean = torch.empty(P, device=cuda) if dev else None
    M = Mb[:, :P] if Mb is not None else None
    plan = eng.sgd_round_plan(W, Xb[:, :P], Yb[:, :P], padded(Gs[0])[:, :P], M, deviation=dev,
                              **opt_kw(opt))
    assert plan is not None and plan["path"] == 1
    out = []
    for i in range(steps):
        G = padded(Gs[i])[:, :P]
        X = Xb[:, :P]
        Y = X if in_place else Yb[:, :P]
        ran = eng.sgd_round(W, X, Y, G, M, LR, first=i == 0, dev_sq=dsq, dev_max=dmax, mean=mean,
                            **opt_kw(opt))
        assert ran is True
        if not in_place:
            Xb, Yb = Yb, Xb
        torch.cuda.synchronize()
        out.append((Xb[:, :P].cpu().numpy(), M.cpu().numpy() if M is not None else None))
    devs = (dsq.cpu().numpy(), float(dmax.item()), mean.cpu().numpy()) if dev else None
    return out, devs, (Xb, Yb, Mb)


def two_launch_steps(cuda, csr, X0, Gs, opt):
    """The parent's sequence on the GPU: dl_sgd_step into S, then dl_mix_round of S."""
    from distributed_learning_amd.workloads import sgd_step
    eng = E()
    W = eng.DeviceCsr(csr, cuda)
    X = dev_t(X0, cuda)
    S, Y = torch.empty_like(X), torch.empty_like(X)
    M = torch.zeros_like(X) if opt[0] != 0.0 else None
    for i, G in enumerate(Gs):
        sgd_step(X, dev_t(G, cuda), M, out=S, lr=LR, first=i == 0, **opt_kw(opt))
        eng.mix_round(W, S, Y)
        X, Y = Y, X
    torch.cuda.synchronize()
    return X.cpu().numpy(), M.cpu().numpy() if M is not None else None


def same(got, want, what):
    assert (got is None) == (want is None), what
    if want is not None:
        assert np.array_equal(bits(got), bits(want)), \
            f"{what}: {np.count_nonzero(bits(got) != bits(want))} of {want.size} elements differ"


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("n,P,deg", SHAPES)
def test_bits_match_the_oracle_and_the_two_launches(cuda, n, P, deg, opt):
    csr, X0, Gs = problem(n, P, deg)
    want = oracle(n, P, deg, opt)
    got, _, _ = fused_steps(cuda, csr, X0, Gs, opt)
    for i in range(STEPS):
        same(got[i][0], want[i][0], f"y, step {i + 1}")
        same(got[i][1], want[i][1], f"buf, step {i + 1}")
    inp, _, _ = fused_steps(cuda, csr, X0, Gs, opt, in_place=True)
    same(inp[-1][0], got[-1][0], "y in place")
    same(inp[-1][1], got[-1][1], "buf in place")
    X2, M2 = two_launch_steps(cuda, csr, X0, Gs, opt)
    same(got[-1][0], X2, "y against dl_sgd_step + dl_mix_round")
    same(got[-1][1], M2, "buf against dl_sgd_step + dl_mix_round")


def test_workgroups_walk_three_tiles(cuda):
    """n_tiles >= 3 x grid (both from dl_sgd_round_plan): the prefetch loop runs more than once
    per workgroup; with a ragged tail tile behind the full ones."""
    eng = E()
    n, deg, opt = 64, 4, OPTS[0]
    csr = graph_csr(n, deg, seed=5)
    W = eng.DeviceCsr(csr, cuda)

    def plan(P):
        t = [torch.empty(n, P, device=cuda) for _ in range(4)]
        return eng.sgd_round_plan(W, t[0], t[1], t[2], t[3], **opt_kw(opt))
    p0 = plan(1 << 20)
    P = 3 * p0["grid"] * p0["tile_cols"] + 4     # (rows stay 16-byte aligned: the float4 kernel)
    assert n * P * 4 <= 256 << 20
    p = plan(P)
    assert p is not None and p["path"] == 1 and p["n_tiles"] >= 3 * p["grid"], p
    rng = np.random.default_rng(1)
    X0 = rng.standard_normal((n, P), dtype=np.float32)
    Gs = [rng.standard_normal((n, P), dtype=np.float32) for _ in range(2)]
    buf = np.zeros_like(X0)
    X = X0
    for i, G in enumerate(Gs):
        X = cref.mix_round(cref.sgd_step(X, G, buf, lr=LR, first=i == 0, **opt_kw(opt)),
                           csr.rowptr, csr.col, csr.w)
    for in_place in (False, True):
        got, _, _ = fused_steps(cuda, csr, X0, Gs, opt, in_place=in_place, steps=2)
        same(got[-1][0], X, f"y (in_place={in_place})")
        same(got[-1][1], buf, f"buf (in_place={in_place})")


@pytest.mark.parametrize("opt", [OPTS[0], OPTS[3]])
@pytest.mark.parametrize("n,P,deg", [(64, 4096, 4), (300, 777, 8)])
def test_tiled_engine_round_sgd(cuda, n, P, deg, opt):
    """GossipEngine(layout="tiled").round_sgd: rows() and M converted back are the row-major
    result's bits."""
    eng = E()
    csr, X0, Gs = problem(n, P, deg)
    want = oracle(n, P, deg, opt)
    g = eng.GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda), layout="tiled")
    assert g.layout == "tiled" and g.order is None
    M = g.layout_like(torch.zeros(n, P)) if opt[0] != 0.0 else None
    for i in range(STEPS):
        G = g.layout_like(dev_t(Gs[i], cuda))
        assert eng.sgd_round_plan(g.W, g.X, g.Y, G, M, tiled=(P, g.T), **opt_kw(opt)) is not None
        g.round_sgd(G, M, LR, first=i == 0, deviation=True, **opt_kw(opt))
    torch.cuda.synchronize()
    same(g.rows().cpu().numpy(), want[-1][0], "rows()")
    if M is not None:
        same(eng.from_tiled(M, P).cpu().numpy(), want[-1][1], "M")
    Y = want[-1][0]
    np.testing.assert_allclose(np.sqrt(g.dev_sq.cpu().numpy()), np.sqrt(cref.deviation_sq(Y)),
                               rtol=DEV_RTOL)


@pytest.mark.parametrize("n,P,deg,weights", [(256, 1030, 4, "regular"), (300, 777, 8, "random"),
                                             (1500, 64, 6, "random"), (64, 4096, 4, "regular"),
                                             (64, 4096, 4, "random"), (1024, 4100, 4, "random")])
def test_deviation(cuda, n, P, deg, weights):
    """dev_sq, dev_max and mean of y: one pass for a doubly stochastic W (uniform weights on a
    regular graph), two passes otherwise."""
    opt = OPTS[0]
    csr, X0, Gs = problem(n, P, deg, weights)
    assert bool(csr.doubly_stochastic) == (weights == "regular")
    want = oracle(n, P, deg, opt, weights)
    got, (dsq, dmax, mean), _ = fused_steps(cuda, csr, X0, Gs, opt, dev=True)
    same(got[-1][0], want[-1][0], "y")
    same(got[-1][1], want[-1][1], "buf")
    check_dev(got[-1][0], dsq, dmax, mean)


# The instantiation families of mix_sgd_tile_kernel that no shape above reaches (tabulated from
# the launch shaping, profiles/r22/tile_core/README.md), each at the agent count that gives it at
# the planner's 32 chunks (1024 / 32 = 32 rows a pass) and 128-column tiles:
#   (n, full tiles, weights, deviation) -> float4 kernel of the full tiles; every launch also runs
#   the guarded kernel on a 5-column tail, with the same deviation form.
# Three tiles are three workgroups of one tile each.  The larger counts exceed the grid (256
# compute units: 129 workgroups for 256 tiles at 8 rows a thread, 257 for 513 at 4), so a
# workgroup walks to a second tile and prefetches it under the first one's mix.
FAMILIES = [(64, 3, "regular", False),     # 2 rows a thread, five-weight rows (reg5), no deviation
            (128, 3, "regular", False),    # 4 rows a thread, reg5, no deviation
            (128, 3, "random", False),     # 4 rows a thread, CSR rows, no deviation
            (128, 3, "regular", True),     # 4 rows a thread, reg5, mean from the inputs
            (256, 3, "random", True),      # 8 rows a thread, two-pass deviation
            (256, 3, "regular", True),     # 8 rows a thread, mean from the inputs
            (128, 513, "random", False),   # the walk: 4 rows a thread, no deviation
            (128, 513, "regular", True),   # the walk: 4 rows a thread, reg5, mean from the inputs
            (256, 256, "random", False),   # the walk: 8 rows a thread, no deviation
            (256, 256, "random", True),    # the walk: 8 rows a thread, two-pass deviation
            (256, 256, "regular", True)]   # the walk: 8 rows a thread, mean from the inputs


def family_params(tiles):
    """Full 128-column tiles and a ragged one of 5; rows 16-byte aligned at ld = P + 3."""
    return tiles * 128 + 5


@pytest.mark.parametrize("n,tiles,weights,dev", FAMILIES)
def test_kernel_families_without_another_case(cuda, n, tiles, weights, dev):
    P, deg, opt = family_params(tiles), 4, OPTS[0]
    csr, X0, Gs = problem(n, P, deg, weights)
    want = oracle(n, P, deg, opt, weights)
    t = [torch.empty(n, P + 3, device=cuda)[:, :P] for _ in range(4)]
    plan = E().sgd_round_plan(E().DeviceCsr(csr, cuda), t[0], t[1], t[2], t[3], deviation=dev,
                              **opt_kw(opt))
    assert plan["tile_cols"] == 128 and plan["n_tiles"] >= tiles, plan
    assert tiles == 3 or plan["grid"] < tiles, plan   # a workgroup walks more than one tile
    got, devs, bufs = fused_steps(cuda, csr, X0, Gs, opt, ld=P + 3, sentinel=-7.25, dev=dev)
    for i in range(STEPS):
        same(got[i][0], want[i][0], f"y, step {i + 1}")
        same(got[i][1], want[i][1], f"buf, step {i + 1}")
    for t in bufs:
        assert torch.all(t[:, P:] == -7.25)
    if dev:
        check_dev(got[-1][0], *devs)


@pytest.mark.parametrize("n,P,deg", [(33, 129, 4), (64, 4096, 4)])
def test_first_step_does_not_read_buf(cuda, n, P, deg):
    opt = OPTS[0]
    csr, X0, Gs = problem(n, P, deg)
    want = oracle(n, P, deg, opt)
    got, _, _ = fused_steps(cuda, csr, X0, Gs, opt, buf_fill=float("nan"), steps=1)
    same(got[0][0], want[0][0], "y")
    same(got[0][1], want[0][1], "buf")


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n,P,deg", [(33, 129, 4), (64, 4096, 4), (300, 777, 8)])
def test_padding_columns_are_never_written(cuda, n, P, deg, in_place):
    """Row-major with ld = P + 4 (129 + 4: rows not 16-byte aligned, the guarded kernel; 4096 + 4:
    the float4 kernel): sentinels in the padding of y and buf survive."""
    opt = OPTS[0]
    csr, X0, Gs = problem(n, P, deg)
    want = oracle(n, P, deg, opt)
    got, _, (Xb, Yb, Mb) = fused_steps(cuda, csr, X0, Gs, opt, in_place=in_place, ld=P + 4,
                                       sentinel=-7.25)
    same(got[-1][0], want[-1][0], "y")
    same(got[-1][1], want[-1][1], "buf")
    for t in (Xb, Yb, Mb):
        assert torch.all(t[:, P:] == -7.25)


def test_fallback_when_the_plan_is_not_path_1(cuda, monkeypatch):
    monkeypatch.setenv("DLAMD_FORCE_GATHER", "1")
    eng = E()
    n, P, deg, opt = 64, 1000, 4, OPTS[0]
    csr, X0, Gs = problem(n, P, deg)
    want = oracle(n, P, deg, opt)
    g = eng.GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda), layout="rows")
    assert g.plan()["path"] == 2 and g.layout == "rows"
    M = g.layout_like(torch.zeros(n, P))
    for i in range(STEPS):
        G = g.layout_like(dev_t(Gs[i], cuda))
        assert eng.sgd_round_plan(g.W, g.X, g.Y, G, M, **opt_kw(opt)) is None   # UNSUPPORTED
        assert eng.sgd_round(g.W, g.X, g.Y, G, M, LR, **opt_kw(opt)) is False
        g.round_sgd(G, M, LR, first=i == 0, deviation=True, **opt_kw(opt))
    torch.cuda.synchronize()
    same(g.rows().cpu().numpy(), want[-1][0], "rows()")
    same(M.cpu().numpy(), want[-1][1], "M")


def test_fallback_in_the_tiled_layout(cuda, monkeypatch):
    """Plan path 4 (the register-CSR kernel) keeps the tiled layout: dl_sgd_step runs over the
    resident buffers as one row each, then the plain round mixes the scratch."""
    monkeypatch.setenv("DLAMD_FORCE_REG", "1")
    eng = E()
    n, P, opt = 1500, 64, OPTS[0]
    csr, X0, Gs = problem(n, P, 4, "regular")
    want = oracle(n, P, 4, opt, "regular")
    g = eng.GossipEngine(csr, P, device=cuda, X=dev_t(X0, cuda))
    assert g.plan()["path"] == 4 and g.layout == "tiled"
    M = g.layout_like(torch.zeros(n, P))
    for i in range(STEPS):
        G = g.layout_like(dev_t(Gs[i], cuda))
        assert eng.sgd_round_plan(g.W, g.X, g.Y, G, M, tiled=(P, g.T), **opt_kw(opt)) is None
        g.round_sgd(G, M, LR, first=i == 0, **opt_kw(opt))
    torch.cuda.synchronize()
    same(g.rows().cpu().numpy(), want[-1][0], "rows()")
    same(eng.from_tiled(M, P).cpu().numpy(), want[-1][1], "M")


@pytest.fixture
def deterministic_convs():
    """MIOpen's default conv solvers are not run-to-run deterministic (tests/test_wrn_gpu.py)."""
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


def test_c5_fused_round_matches_the_two_launches(cuda, deterministic_convs):
    """WRNConsensusSGD(fused_round=True) against fused_round=False from the same X0, data and
    labels: two eager steps, capture, two replayed steps."""
    from distributed_learning_amd.graph import Csr
    from distributed_learning_amd.workloads import WRNConsensusSGD
    from oracle import mixer_ref
    n, B, arch = 4, 6, (10, 1, 0.0, 10)
    topo = {0: {0: 0.5, 1: 0.25, 3: 0.25}, 1: {1: 0.6, 0: 0.25, 2: 0.15},
            2: {2: 0.6, 1: 0.15, 3: 0.25}, 3: {3: 0.5, 2: 0.25, 0: 0.25}}
    rp, cols, w = mixer_ref.topology_to_csr(topo)
    csr = Csr(rp, cols, w)
    g = torch.Generator().manual_seed(3)
    data = torch.randn(n, B, 3, 32, 32, generator=g).to(cuda)
    labels = torch.randint(0, 10, (n, B), generator=g).to(cuda)
    kw = dict(lr=0.05, momentum=0.9, weight_decay=5e-4, device=cuda, seed=7, streams=1,
              data=data, labels=labels)
    a = WRNConsensusSGD(csr, B, *arch, fused_round=False, **kw)
    X0 = a.params().cpu().numpy().copy()
    b = WRNConsensusSGD(csr, B, *arch, fused_round=True, X0=X0, **kw)
    assert b.fused_round and b.S is None and a.S is not None and not a.fused_round
    assert torch.equal(a.params(), b.params())
    for wl in (a, b):
        wl.step()
        wl.step()
    for wl in (a, b):
        wl.capture()
    for wl in (a, b):
        wl.replay(2)
    torch.cuda.synchronize()
    assert a.steps_done == b.steps_done == 4
    assert torch.equal(a.params(), b.params())
    assert torch.equal(a.M, b.M) and torch.equal(a.loss, b.loss)
    assert not b.X[:, b.P:].any()
    np.testing.assert_allclose(np.sqrt(b.dev_sq.cpu().numpy()), np.sqrt(a.dev_sq.cpu().numpy()),
                               rtol=DEV_RTOL)
    # the module parameters are still views of X's rows
    assert next(b.models[1].parameters()).data_ptr() == b.X[1].data_ptr()
