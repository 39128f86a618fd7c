"""NaN, infinities, subnormals, signed zeros and near-overflow values through the mixing kernels:
every path holds ``same_bits`` against the oracle its ordinary test uses (cref.mix_round,
cref.sgd_step, tests/cheb_oracle.py, numpy for dl_axpby), and every deviation output has the
class (finite, inf, NaN) of cref.deviation_sq of the oracle's output -- a max deviation is
np.max(np.sqrt(dev_sq)): NaN when any agent's is.  Inputs: tests/special_values.py, whose
properties tests/test_special_values_cpu.py checks without a GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cheb_oracle as O
import special_values as sv
from oracle import cref
from oracle import mixer_ref as M
from test_mix_gpu import DEV_RTOL, dev_floor

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CLS = pytest.mark.parametrize("cls", sv.CLASSES)
SGD = pytest.mark.parametrize("sgd", [False, True])


def E():
    from distributed_learning_amd import engine
    return engine


def dev_t(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)


def host(t):
    return t.detach().cpu().numpy()


def assert_bits(got, want, what=""):
    assert sv.same_bits(got, want), f"{what}: {sv.describe(got, want)}"


def oracle_round(case, sgd):
    with np.errstate(all="ignore"):
        return cref.mix_round(case.X, case.csr.rowptr, case.csr.col, case.csr.w,
                              G=case.G if sgd else None, lr=case.lr if sgd else 0.0)


def assert_max(got, Y, what=""):
    """got against np.max(np.sqrt(dev_sq)) of the oracle's Y: NaN, inf, or within DEV_RTOL and
    the mean-rounding floor of tests/test_mix_gpu.py."""
    want = sv.dev_max32(Y)
    got = np.float32(got)
    if np.isnan(want):
        assert np.isnan(got), f"{what}: max deviation {got!r}, the oracle's is NaN"
    elif np.isinf(want):
        assert got == want, f"{what}: max deviation {got!r}, the oracle's is inf"
    else:
        with np.errstate(all="ignore"):
            floor = dev_floor(M.column_mean(Y), Y.shape[1])
        print(f"{what}: max deviation {got!r} oracle {want!r} floor {floor:.3e}")
        assert got == pytest.approx(float(np.sqrt(cref.deviation_sq(Y).max())), rel=DEV_RTOL,
                                    abs=floor), what


def assert_dev(Y, dsq, dmax, mean=None, what=""):
    """dev_sq / dev_max / mean of a launch against the oracle's output Y."""
    with np.errstate(all="ignore"):
        want64 = cref.deviation_sq(Y)
        want = want64.astype(np.float32)
        want_mean = M.column_mean(Y)
    cls, got_cls = sv.classes_of(want), sv.classes_of(dsq)
    bad = np.flatnonzero(cls != got_cls)
    assert not len(bad), (f"{what}: dev_sq class (0 finite, 1 inf, 3 NaN) differs at agents "
                          f"{bad[:8]}: got {got_cls[bad[:8]]} want {cls[bad[:8]]}")
    fin = cls == 0
    if fin.any():
        floor = dev_floor(want_mean, Y.shape[1])    # (a finite deviation: the mean is finite)
        np.testing.assert_allclose(np.sqrt(dsq[fin]), np.sqrt(want64[fin]), rtol=DEV_RTOL,
                                   atol=floor, err_msg=what)
    assert_max(dmax, Y, what)
    if mean is not None:
        mcls = sv.classes_of(want_mean)
        bad = np.flatnonzero(sv.classes_of(mean) != mcls)
        assert not len(bad), (f"{what}: mean class differs at columns {bad[:8]}: got "
                              f"{mean[bad[:8]]} want {want_mean[bad[:8]]}")
        f = mcls == 0
        # tests/test_mix_gpu.py's bound for a mean (rtol 1e-5, atol 1e-6) is for columns of
        # ordinary values.  A column that holds +-1e38 entries which cancel has a mean of
        # ordinary size and a sum whose rounding error is set by the entries: two fp32 sums of n
        # terms in different orders differ by at most 2 (n - 1) eps sum|y_i|, their means by
        # 2 (n - 1) eps mean|y_i| (Higham, Accuracy and Stability, eq. 4.4).  That bound is
        # used for columns holding an entry above 2^100, the other columns keep the suite's.
        n = Y.shape[0]
        with np.errstate(all="ignore"):
            big = np.abs(Y).max(axis=0) > 2.0 ** 100
            err = 2.0 * (n - 1) * np.finfo(np.float32).eps * \
                np.abs(Y.astype(np.float64)).mean(axis=0)
        atol = np.where(big, err, 1e-6)[f]
        miss = np.abs(mean[f].astype(np.float64) - want_mean[f]) > 1e-5 * np.abs(want_mean[f]) + atol
        assert not miss.any(), (f"{what}: mean differs at columns {np.flatnonzero(f)[miss][:8]}: "
                                f"got {mean[f][miss][:8]} want {want_mean[f][miss][:8]}")


# ---------------------------------------------------------------- dl_mix_round
def run_rows(cuda, case, sgd, path):
    """dl_mix_round on row-major operands; the plan query must name ``path``."""
    e = E()
    n, P = case.X.shape
    W = e.DeviceCsr(case.csr, cuda)
    assert e.plan_shape(W, P, deviation=True)["path"] == path
    X, G = dev_t(case.X, cuda), dev_t(case.G, cuda) if sgd else None
    Y = torch.empty_like(X)
    assert e.mix_plan(W, X, Y, G, deviation=True)["path"] == path
    dsq, dmax, mean = torch.empty(n, device=cuda), torch.empty(1, device=cuda), \
        torch.empty(P, device=cuda)
    e.mix_round(W, X, Y, G=G, lr=case.lr if sgd else 0.0, dev_sq=dsq, dev_max=dmax, mean=mean)
    torch.cuda.synchronize()
    return host(Y), host(dsq), float(dmax.item()), host(mean)


@CLS
@SGD
@pytest.mark.parametrize("name", ["small_8x37", "rows_64x256"])
def test_mix_round_row_major(cuda, name, sgd, cls):
    """The LDS tile kernel on row-major operands: 8 x 37 (one tile, the guarded unaligned
    tail) and 64 x 256 (float4 tiles)."""
    case = sv.shape_case(name, cls)
    Y, dsq, dmax, mean = run_rows(cuda, case, sgd, 1)
    want = oracle_round(case, sgd)
    assert_bits(Y, want, "y")
    assert_dev(want, dsq, dmax, mean, "deviation")


@CLS
@SGD
def test_mix_round_gather(cuda, monkeypatch, sgd, cls):
    monkeypatch.setenv("DLAMD_FORCE_GATHER", "1")
    case = sv.shape_case("gather_64x1000", cls)
    Y, dsq, dmax, mean = run_rows(cuda, case, sgd, 2)
    want = oracle_round(case, sgd)
    assert_bits(Y, want, "y")
    assert_dev(want, dsq, dmax, mean, "deviation")


def engine_round(cuda, case, sgd, layout, path, T=None):
    e = E()
    n, P = case.X.shape
    eng = e.GossipEngine(case.csr, P, device=cuda, X=dev_t(case.X, cuda), layout=layout,
                         tile_cols=T)
    plan = eng.plan()
    assert plan["path"] == path and eng.layout == layout, plan
    if T:
        assert plan["tile_cols"] == T, plan
    mean = torch.empty(P, device=cuda)
    eng.round(G=eng.layout_like(dev_t(case.G, cuda)) if sgd else None,
              lr=case.lr if sgd else 0.0, deviation=True, mean=mean)
    torch.cuda.synchronize()
    return host(eng.rows()), host(eng.agent_dev_sq()), float(eng.dev_max.item()), host(mean)


@CLS
@SGD
@pytest.mark.parametrize("T", [4, 64])
def test_mix_round_column_tiled(cuda, T, sgd, cls):
    case = sv.shape_case("rows_64x256", cls)
    Y, dsq, dmax, mean = engine_round(cuda, case, sgd, "tiled", 1, T)
    want = oracle_round(case, sgd)
    assert_bits(Y, want, "y")
    assert_dev(want, dsq, dmax, mean, "deviation")


@CLS
@SGD
@pytest.mark.parametrize("layout", ["tiled", "rows"])
@pytest.mark.parametrize("name,path", [("reg4_64x64", 4), ("reg5_64x64", 5)])
def test_mix_round_register_csr(cuda, monkeypatch, name, path, layout, sgd, cls):
    """The register-CSR tile kernels (path 4: regular, path 5: register head + LDS tail) on the
    64-agent fixture graphs, forced as tests/test_mix_ragged_gpu.py forces them."""
    monkeypatch.setenv("DLAMD_FORCE_REG", "1")
    case = sv.shape_case(name, cls)
    Y, dsq, dmax, mean = engine_round(cuda, case, sgd, layout, path)
    want = oracle_round(case, sgd)
    assert_bits(Y, want, "y")
    assert_dev(want, dsq, dmax, mean, "deviation")


@CLS
@pytest.mark.parametrize("force_gather", [False, True])
def test_halo_rows(cuda, monkeypatch, force_gather, cls):
    """Local rows + halo rows already stepped by dl_step_rows, as a remote rank sends them
    (tests/test_mix_gpu.py::test_halo_rows_equal_full_mix): the local rows of the full round."""
    from distributed_learning_amd.graph import Csr
    if force_gather:
        monkeypatch.setenv("DLAMD_FORCE_GATHER", "1")
    e = E()
    case = sv.shape_case("halo_40x70", cls)
    n, P = case.X.shape
    n_loc = 24
    full = case.csr
    want = oracle_round(case, True)
    local = Csr(full.rowptr[:n_loc + 1], full.col[:full.rowptr[n_loc]],
                full.w[:full.rowptr[n_loc]], n_src=n)
    Xd, Gd = dev_t(case.X, cuda), dev_t(case.G, cuda)
    rows = torch.arange(n_loc, n, dtype=torch.int32, device=cuda)
    halo = torch.empty(n - n_loc, P, device=cuda)
    e.step_rows(Xd, rows, halo, G=Gd, lr=case.lr)
    with np.errstate(all="ignore"):
        assert_bits(host(halo), M.sgd_step(case.X, case.G, case.lr)[n_loc:], "dl_step_rows")
    W = e.DeviceCsr(local, cuda)
    Y = torch.empty(n_loc, P, device=cuda)
    e.mix_round(W, Xd[:n_loc], Y, G=Gd[:n_loc], lr=case.lr, halo=halo)
    torch.cuda.synchronize()
    assert_bits(host(Y), want[:n_loc], "y")


# ---------------------------------------------------------------- dl_mix_rounds, k = 3
K = 3


def oracle_rounds(case, sgd, k=K):
    """[Y after round 1..k]: the local step before the first round only."""
    out = [oracle_round(case, sgd)]
    with np.errstate(all="ignore"):
        for _ in range(k - 1):
            out.append(cref.mix_round(out[-1], case.csr.rowptr, case.csr.col, case.csr.w))
    return out


@CLS
@SGD
@pytest.mark.parametrize("name,layout,dev", [("rounds_64x4096", "tiled", False),
                                             ("rounds_100x1024", "rows", False),
                                             ("rounds_rr64x256", "tiled", True)])
def test_mix_rounds(cuda, name, layout, dev, sgd, cls):
    """Three rounds in one pass.  The multi-round kernel fuses the final deviation only for a
    doubly stochastic W (dl_mix_rounds_plan refuses it otherwise), so the two shapes on random
    directed graphs run without it and a random 4-regular graph with its best constant weight
    runs with it."""
    e = E()
    case = sv.shape_case(name, cls)
    n, P = case.X.shape
    eng = e.GossipEngine(case.csr, P, device=cuda, X=dev_t(case.X, cuda), layout=layout)
    assert eng.layout == layout
    tiled = (eng.P, eng.T) if layout == "tiled" else None
    plan = e.rounds_plan(eng.W, eng.X, eng.Y, deviation=dev, tiled=tiled)
    assert plan is not None and plan["path"] == 3, plan
    assert bool(case.csr.doubly_stochastic) == dev
    mean = torch.empty(P, device=cuda) if dev else None
    eng.rounds(K, G=eng.layout_like(dev_t(case.G, cuda)) if sgd else None,
               lr=case.lr if sgd else 0.0, deviation=dev, mean=mean)
    torch.cuda.synchronize()
    want = oracle_rounds(case, sgd)[-1]
    assert_bits(host(eng.rows()), want, "y")
    if dev:
        assert_dev(want, host(eng.agent_dev_sq()), float(eng.dev_max.item()), host(mean),
                   "deviation")


# ---------------------------------------------------------------- dl_mix_rounds_trace, k = 3
def run_trace(cuda, case):
    e = E()
    W = e.DeviceCsr(case.csr, cuda)
    X = dev_t(case.X, cuda)
    Y = torch.full_like(X, 7.0)
    assert e.trace_max_rounds(W, X, Y) >= 4
    tr = torch.full((K,), -1.0, device=cuda)
    e.mix_rounds_trace(W, X, Y, K, tr)
    torch.cuda.synchronize()
    assert_bits(host(X), case.X, "the pass input")
    return host(Y), host(tr)


def check_trace(case, Y, tr):
    want = oracle_rounds(case, False)
    assert_bits(Y, want[-1], "y")
    for i in range(K):
        assert_max(tr[i], want[i], f"trace[{i}]")


@CLS
@pytest.mark.parametrize("planes", [False, True])
def test_mix_rounds_trace_regular(cuda, monkeypatch, planes, cls):
    """Both kernels of test_trace_rows_and_planes_kernels_agree: the agent-major one (default
    for register-cached regular graphs) and the chunk-major planes kernel."""
    if planes:
        monkeypatch.setenv("DLAMD_TRACE_PLANES", "1")
    case = sv.shape_case("trace_rr300x256", cls)
    assert case.csr.doubly_stochastic and case.csr.uniform_row_nnz == 5
    check_trace(case, *run_trace(cuda, case))


@CLS
def test_mix_rounds_trace_irregular(cuda, cls):
    """The "metro" case of tests/test_mix_trace_gpu.py (irregular, CSR in LDS)."""
    case = sv.shape_case("trace_metro50x1000", cls)
    assert case.csr.doubly_stochastic and not case.csr.uniform_row_nnz
    check_trace(case, *run_trace(cuda, case))


# ---------------------------------------------------------------- dl_mix_until
def until_oracle(case, times, eps, max_rounds):
    """dl_mix_until's loop (include/dlamd.h) on the oracle: (y, rounds, status word 1, trace)."""
    rp, cl, w = case.csr.rowptr, case.csr.col, case.csr.w
    X, done, outs = case.X, 0, [case.X]
    eps32 = None if eps is None else np.float32(eps)

    def test(Z):
        if eps is None:
            return done >= times, False
        d = sv.dev_max32(Z)
        return bool(d < eps32) and done >= times, bool(np.isnan(d))
    stop, nan = test(X)
    while not stop and not nan and done < max_rounds:
        with np.errstate(all="ignore"):
            X = cref.mix_round(X, rp, cl, w)
        done += 1
        outs.append(X)
        stop, nan = test(X)
    return X, done, 1 if stop else 2 if nan else 0, outs


@CLS
@pytest.mark.parametrize("times,eps,max_rounds", [(3, None, 4096), (1, 1e-3, 4)])
@pytest.mark.parametrize("name", ["until_5x617", "until_16x63", "until_3x1"])
def test_mix_until(cuda, name, times, eps, max_rounds, cls):
    """times = 3 without eps, and eps with max_rounds = 4: the iterate, the round count, the
    status word (2: the stop test met a NaN, the loop ended there) and every traced max
    deviation.  In until_3x1, tiny, all three values are subnormal: every (x - mean)^2 underflows
    in fp32 (a max deviation of 0.0 against the oracle's 7.803e-39), which is why the kernel
    takes a row's norm again in fp64 where its fp32 sum of squares is below 2^-100."""
    e = E()
    case = sv.shape_case(name, cls)
    n, P = case.X.shape
    W = e.DeviceCsr(case.csr, cuda)
    assert e.until_fits(W, P)
    X = dev_t(case.X, cuda)
    status = torch.full((2,), -1, dtype=torch.int32, device=cuda)
    trace = torch.full((max_rounds + 1,), -1.0, device=cuda)
    e.mix_until(W, X, X, times, eps, max_rounds, status, trace)
    torch.cuda.synchronize()
    want, want_n, want_s, outs = until_oracle(case, times, eps, max_rounds)
    got_n, got_s = status.tolist()
    assert (got_n, got_s) == (want_n, want_s)
    assert_bits(host(X), want, "y")
    if eps is not None:
        tr = host(trace)
        for i, Z in enumerate(outs):
            assert_max(tr[i], Z, f"dev_trace[{i}]")


# ---------------------------------------------------------------- dl_sgd_round, dl_cheb_round
OPT = dict(momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=True)
FUSED = [("fused_33x129", "rows"), ("fused_circ64x256", "tiled")]


def second_gradient(case):
    """A second step's gradients: the first's, rows rolled by one (special values included)."""
    return np.roll(case.G, 1, axis=0)


@CLS
@pytest.mark.parametrize("name,layout", FUSED)
def test_sgd_round(cuda, name, layout, cls):
    """Momentum, Nesterov and weight decay on; first = 1, then first = 0 on the carried buffers:
    y and the buffers against cref.sgd_step then cref.mix_round, the deviation of each y."""
    e = E()
    case = sv.shape_case(name, cls)
    n, P = case.X.shape
    rp, cl, w = case.csr.rowptr, case.csr.col, case.csr.w
    g = e.GossipEngine(case.csr, P, device=cuda, X=dev_t(case.X, cuda), layout=layout)
    assert g.layout == layout
    tiled = (P, g.T) if layout == "tiled" else None
    Mb = g.layout_like(torch.zeros(n, P, device=cuda))
    Xw, buf = case.X, np.zeros_like(case.X)
    for i, Gh in enumerate([case.G, second_gradient(case)]):
        G = g.layout_like(dev_t(Gh, cuda))
        plan = e.sgd_round_plan(g.W, g.X, g.Y, G, Mb, deviation=True, tiled=tiled, **OPT)
        assert plan is not None and plan["path"] == 1, plan
        mean = torch.empty(P, device=cuda)
        assert e.sgd_round(g.W, g.X, g.Y, G, Mb, case.lr, first=i == 0, dev_sq=g.dev_sq,
                           dev_max=g.dev_max, mean=mean, workspace=g.ws, tiled=tiled,
                           **OPT) is True
        g.X, g.Y = g.Y, g.X
        torch.cuda.synchronize()
        with np.errstate(all="ignore"):
            S = cref.sgd_step(Xw, Gh, buf, lr=case.lr, first=i == 0, **OPT)
            Xw = cref.mix_round(S, rp, cl, w)
        assert_bits(host(g.rows()), Xw, f"y, step {i + 1}")
        Mh = host(e.from_tiled(Mb, P)) if tiled else host(Mb)
        assert_bits(Mh, buf, f"buf, step {i + 1}")
        assert_dev(Xw, host(g.agent_dev_sq()), float(g.dev_max.item()), host(mean),
                   f"deviation, step {i + 1}")


@CLS
@pytest.mark.parametrize("name,layout", FUSED)
def test_cheb_round(cuda, name, layout, cls):
    """Two rounds y = a W x + b z (y = z, the loop's mode) with tests/cheb_oracle.py's rule; z
    is the case's G: a matrix of the same class, unrelated to x.  a = 1.5 first, the suite's own
    first coefficient (tests/test_cheb_round_gpu.py) and a value the Chebyshev weights take.

    fused_circ64x256, tiled, huge is the case the kernel's fallback is for: W is doubly
    stochastic, so mean(y) comes from the inputs as mean(a x + b z), and in the column where
    +3e38 and -3e38 meet 1.5 * 3e38 is +inf, 1.5 * -3e38 is -inf and their sum NaN, against a
    numpy mean of y of 0.00188812.  A tile whose input mean is not finite takes the two-pass
    form (the mean summed from y), include/dlamd.h."""
    e = E()
    case = sv.shape_case(name, cls)
    n, P = case.X.shape
    rp, cl, w = case.csr.rowptr, case.csr.col, case.csr.w
    g = e.GossipEngine(case.csr, P, device=cuda, X=dev_t(case.X, cuda), layout=layout)
    assert g.layout == layout
    tiled = (P, g.T) if layout == "tiled" else None
    g.Y = g.layout_like(dev_t(case.G, cuda))
    Xw, Zw = case.X, case.G
    for i, (a, b) in enumerate([(1.5, -0.5), (0.75, 0.5)]):
        plan = e.cheb_round_plan(g.W, g.X, g.Y, g.Y, deviation=True, tiled=tiled)
        assert plan is not None and plan["path"] == 1, plan
        mean = torch.empty(P, device=cuda)
        assert e.cheb_round(g.W, g.X, g.Y, g.Y, a, b, dev_sq=g.dev_sq, dev_max=g.dev_max,
                            mean=mean, workspace=g.ws, tiled=tiled) is True
        g.X, g.Y = g.Y, g.X
        torch.cuda.synchronize()
        with np.errstate(all="ignore"):
            Xw, Zw = O.cheb_step(cref.mix_round(Xw, rp, cl, w), Zw, a, b), Xw
        assert_bits(host(g.rows()), Xw, f"y, round {i + 1}")
        assert_dev(Xw, host(g.agent_dev_sq()), float(g.dev_max.item()), host(mean),
                   f"deviation, round {i + 1}")


# ---------------------------------------------------------------- the element-wise kernels
@CLS
@pytest.mark.parametrize("P", [256, 37])
def test_sgd_step(cuda, P, cls):
    """dl_sgd_step, float4 (P = 256) and scalar (P = 37) forms, first = 1 then first = 0."""
    from distributed_learning_amd.workloads import sgd_step
    from test_mix_gpu import graph_csr
    case = sv.build(cls, 8, P, graph_csr(8, 3, seed=8), seed=P)
    X, Mb = dev_t(case.X, cuda), torch.zeros(8, P, device=cuda)
    Xw, buf = case.X, np.zeros_like(case.X)
    for i, Gh in enumerate([case.G, second_gradient(case)]):
        out = torch.empty_like(X)
        sgd_step(X, dev_t(Gh, cuda), Mb, out=out, lr=case.lr, first=i == 0, **OPT)
        torch.cuda.synchronize()
        with np.errstate(all="ignore"):
            Xw = cref.sgd_step(Xw, Gh, buf, lr=case.lr, first=i == 0, **OPT)
        assert_bits(host(out), Xw, f"out, step {i + 1}")
        assert_bits(host(Mb), buf, f"buf, step {i + 1}")
        X = out
    if cls == "tiny":   # (the plain step x - lr g keeps the -0.0 of the class's second feature)
        out = torch.empty_like(X)
        sgd_step(dev_t(case.X, cuda), dev_t(case.G, cuda), None, out=out, lr=case.lr)
        want = cref.sgd_step(case.X, case.G, None, lr=case.lr)
        assert (sv.bits(want) == 0x80000000).any()
        assert_bits(host(out), want, "plain step")


@pytest.mark.parametrize("P", [256, 37])
def test_axpby(cuda, P):
    """dl_axpby against numpy's fl(fl(a s) + fl(b z)), float4 and scalar forms: NaN and inf in s
    only, in z only, a = 0 or b = 0 against an inf (0 * inf = NaN), and the tiny and huge values
    (an overflowing product, a subnormal one, signed zeros)."""
    e = E()
    f = np.float32
    rng = np.random.default_rng(P)
    n = 6
    s0 = rng.standard_normal((n, P), dtype=f)
    z0 = rng.standard_normal((n, P), dtype=f)
    specials = [f("nan"), f("inf"), f("-inf"), f(3e38), f(-3e38), sv.MIN_SUB, -sv.MAX_SUB,
                f(6e-39), f(-0.0), f(0.0), sv.MIN_NORM]
    for a, b in [(1.5, -0.5), (0.0, 1.0), (1.0, 0.0), (0.0, 0.0), (-0.25, 0.25)]:
        for where in ("s", "z", "both"):
            s, z = s0.copy(), z0.copy()
            for j, v in enumerate(specials):
                c = (j * (P - 1)) // (len(specials) - 1)
                if where in ("s", "both"):
                    s[j % n, c] = v
                if where in ("z", "both"):
                    z[(j + 1) % n, c] = v
            got = e.axpby(dev_t(s, cuda), dev_t(z, cuda), a, b)
            torch.cuda.synchronize()
            with np.errstate(all="ignore"):
                want = f(a) * s + f(b) * z
            assert_bits(host(got), want, f"a={a} b={b} specials in {where}")


@CLS
def test_step_rows_and_tiled_peers(cuda, cls):
    """dl_step_rows (row-major) and dl_step_rows_tiled_peers (column-tiled, two peers) against
    numpy's fl(x - fl(lr g)), with and without g."""
    from test_mix_gpu import graph_csr
    e = E()
    n, P, T = 24, 72, 8
    case = sv.build(cls, n, P, graph_csr(n, 3, seed=24), seed=5)
    X, G = dev_t(case.X, cuda), dev_t(case.G, cuda)
    sel = np.random.default_rng(1).permutation(n)[:13].astype(np.int32)
    rows = torch.from_numpy(sel).to(cuda)
    with np.errstate(all="ignore"):
        stepped = M.sgd_step(case.X, case.G, case.lr)
    for with_g in (True, False):
        want = (stepped if with_g else case.X)[sel]
        out = torch.full((len(sel), P), 7.0, device=cuda)
        e.step_rows(X, rows, out, G=G if with_g else None, lr=case.lr)
        torch.cuda.synchronize()
        assert_bits(host(out), want, f"dl_step_rows, g {with_g}")
        Xt, Gt = e.to_tiled(X, T), e.to_tiled(G, T)
        sizes = [5, 8]
        outs = [torch.full((P // T, k, T), 7.0, device=cuda) for k in sizes]
        e.step_rows_tiled_peers(Xt, rows, [0, 5, 13], outs, G=Gt if with_g else None, lr=case.lr)
        torch.cuda.synchronize()
        for b, (lo, hi) in enumerate([(0, 5), (5, 13)]):
            got = host(outs[b]).transpose(1, 0, 2).reshape(hi - lo, P)
            assert_bits(got, want[lo:hi], f"dl_step_rows_tiled_peers, peer {b}, g {with_g}")


@CLS
@pytest.mark.parametrize("T", [4, 64])
def test_tiled_round_trip_is_a_copy(cuda, T, cls):
    """dl_to_tiled / dl_from_tiled: the bits are unchanged, NaN sign and payload included."""
    from test_mix_gpu import graph_csr
    e = E()
    n, P = 8, 37 if T == 4 else 200
    case = sv.build(cls, n, P, graph_csr(n, 3, seed=8), seed=T)
    X = case.X.copy()
    X[3, P - 1] = np.uint32(0xFFC12345).view(np.float32)      # negative quiet NaN with a payload
    X[5, 0] = np.uint32(0x7FA00001).view(np.float32)          # a signalling NaN
    Xt = e.to_tiled(dev_t(X, cuda), T)
    back = e.from_tiled(Xt, P)
    torch.cuda.synchronize()
    tiles = -(-P // T)
    padded = np.zeros((n, tiles * T), np.float32)
    padded[:, :P] = X
    want_t = padded.reshape(n, tiles, T).transpose(1, 0, 2)
    assert np.array_equal(sv.bits(host(Xt)), sv.bits(want_t))
    assert np.array_equal(sv.bits(host(back)), sv.bits(X))


# ---------------------------------------------------------------- the reductions, by position
ROWS = [0, 63, 64, 129]    # first and last lane of a wave, the next wave, the next workgroup


@pytest.mark.parametrize("n_parts", [1, 17, 130])
@pytest.mark.parametrize("r", ROWS)
def test_row_sums_nan_position(cuda, n_parts, r):
    e = E()
    n = 130
    parts = np.random.default_rng(n_parts + r).random((n_parts, n), dtype=np.float32)
    parts[(n_parts * 2) // 3, r] = np.nan
    Pd = dev_t(parts, cuda)
    want = parts.astype(np.float64).sum(0).astype(np.float32)
    others = np.arange(n) != r
    for zeroed in (False, True):
        sums = torch.full((n,), 7.0, device=cuda)
        mx = torch.zeros(1, device=cuda) if zeroed else torch.full((1,), 7.0, device=cuda)
        e.row_sums(Pd, sums, mx, max_zeroed=zeroed)
        torch.cuda.synchronize()
        got = host(sums)
        assert np.isnan(got[r])
        np.testing.assert_allclose(got[others], want[others], rtol=1e-6)
        assert np.isnan(mx.item()), (zeroed, mx.item())


@pytest.mark.parametrize("r", ROWS)
def test_deviation_nan_in_one_agent(cuda, r):
    """dl_deviation with a finite mean_in: only the agent that holds the NaN has a NaN dev_sq,
    and dev_max is NaN."""
    e = E()
    n, P = 130, 100
    rng = np.random.default_rng(r)
    X = rng.standard_normal((n, P), dtype=np.float32)
    mean = M.column_mean(X)
    X[r, (r * 7) % P] = np.nan
    dsq, dmax = e.deviation(dev_t(X, cuda), mean_in=dev_t(mean, cuda))
    torch.cuda.synchronize()
    got = host(dsq)
    want = cref.deviation_sq(X, mean)
    others = np.arange(n) != r
    assert np.isnan(got[r]) and np.isnan(want[r])
    np.testing.assert_allclose(np.sqrt(got[others]), np.sqrt(want[others]), rtol=DEV_RTOL,
                               atol=dev_floor(mean, P))
    assert np.isnan(dmax.item())


@pytest.mark.parametrize("value", [np.nan, np.inf])
@pytest.mark.parametrize("c", [0, 255, 256, 599])
def test_max_column_std_poisoned_column(cuda, c, value):
    """One NaN, or one +inf, in one column of 7 x 600: numpy's std of that column is NaN, and
    the maximum over columns keeps it."""
    e = E()
    X = np.random.default_rng(c).standard_normal((7, 600), dtype=np.float32)
    X[c % 7, c] = value
    with np.errstate(all="ignore"):
        assert np.isnan(X.std(axis=0).max())
    assert np.isnan(e.max_column_std(dev_t(X, cuda)).item())


def test_column_sum_special_columns(cuda):
    e = E()
    n, P = 7, 600
    X = np.random.default_rng(0).standard_normal((n, P), dtype=np.float32)
    X[2, 0] = np.nan
    X[6, 255] = np.inf
    X[0, 256], X[5, 256] = np.inf, -np.inf
    X[:, 300] = 3e38
    X[1, 599], X[2, 599] = -np.inf, -0.0
    X[:, 17] = -0.0
    X[:, 18] = sv.MIN_SUB
    with np.errstate(all="ignore"):
        want = np.add.reduce(X, axis=0)
        seq = np.zeros(P, np.float32)
        for r in range(n):
            seq = seq + X[r]
    assert sv.same_bits(want, seq)      # numpy adds the rows in order, from +0.0
    got = host(e.column_sum(dev_t(X, cuda)))
    assert_bits(got, want, "column sums")
    assert sv.bits(got)[17] == 0            # a column of -0.0 sums to +0.0, as numpy's


# ---------------------------------------------------------------- the Mixer, in a child process
def test_mixer_nan_raises_and_leaves_models(cuda, tmp_path):
    """Mixer on models holding one NaN weight: get_max_parameters_std() and every
    get_parameters_deviation() are NaN, mix(times=1, eps=1e-3) raises FloatingPointError and
    leaves the models' bits alone -- the 4-agent TOPO of tests/test_mixer_gpu.py (the
    one-launch route) and 1100 agents (the traced / round-loop route), there also with an
    overflow that turns the deviation NaN only after the first round.  A half-applied fix would
    loop for ever here, so this runs in a child process with a time limit, and only once the
    pieces it rests on hold in this process: the host's decision, the NaN-keeping device
    maximum and dl_mix_until's NaN status, each one bounded launch."""
    from distributed_learning_amd.stop_rule import below_eps
    from test_mix_gpu import graph_csr
    e = E()
    with pytest.raises(FloatingPointError):
        below_eps(np.float32("nan"), 1e-3, 0)
    X = np.random.default_rng(0).standard_normal((4, 8), dtype=np.float32)
    X[2, 3] = np.nan
    _, dmax = e.deviation(dev_t(X, cuda))
    assert np.isnan(dmax.item())
    status = torch.full((2,), -1, dtype=torch.int32, device=cuda)
    Xd = dev_t(X, cuda)
    e.mix_until(e.DeviceCsr(graph_csr(4, 2, seed=1, weights="uniform"), cuda), Xd, Xd, 1, 1e-3, 4,
                status, torch.empty(5, device=cuda))
    assert status.tolist() == [0, 2]
    dst = str(tmp_path / "out.json")
    r = subprocess.run([sys.executable, os.path.join(HERE, "special_mixer_child.py"), dst],
                       timeout=150, capture_output=True, text=True)
    assert r.returncode == 0, f"child exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    with open(dst) as f:
        out = json.load(f)
    assert sorted(out) == ["n1100_nan", "n1100_overflow", "n4_nan"]
    for name, res in out.items():
        assert res["raised"] == "FloatingPointError" and "round" in res["message"], (name, res)
        assert res["bits_unchanged"], (name, res)
    for name in ("n4_nan", "n1100_nan"):
        assert out[name]["std_is_nan"] and out[name]["all_devs_nan"], (name, out[name])
        assert "after round 0" in out[name]["message"], (name, out[name])
    assert out["n4_nan"]["route"] == "resident"
    # 3e38 is a number: its deviations before the call are inf, the NaN comes with the rounds
    assert not out["n1100_overflow"]["all_devs_nan"]
    assert "after round 0" not in out["n1100_overflow"]["message"]
    assert out["n1100_overflow"]["route"] in ("traced", "loop")
