"""GPU parity of dl_cheb_rounds with its definition restated in numpy fp32: the CSR-order left fold
from +0.0, then u_{r+1} = fl(fl(a fold) + fl(b u_{r-1})).  One sequence u_1 .. u_10 per graph
serves every case: a first pass of K rounds must give u_K and u_{K-1}, a pass of K rounds continued
from (u_3, u_2) u_{3+K} and u_{2+K}, bit for bit; trace and deviation of both within 1e-5 relative
or the mean-rounding floor of fp64 deviations of the iterates."""
import functools

import numpy as np
import pytest
import torch

from test_mix_gpu import DEV_RTOL, bits, dev_floor, shared_weight_graph

pytestmark = pytest.mark.gpu

KS, SPLIT = [1, 2, 3, 7], 3   # SPLIT: rounds before the continued pass
N_SEQ = SPLIT + max(KS)


@functools.lru_cache(maxsize=None)
def graph(name):
    """(csr, column-tiled width, columns, traced): each at a P of more tiles than workgroups.
    Rows per thread KV = ceil(agents x width / 4096) rounded up to 2, 4, 8."""
    from distributed_learning_amd import graph as G
    if name == "reg1024":    # register CSR, KV 4, N fills every slot: unguarded, old from LDS
        return shared_weight_graph(1024, seed=3), 16, 16 * 600, True
    if name == "reg512":     # register CSR, KV 2, unguarded: old[k] in registers, z prefetched
        return shared_weight_graph(512, seed=4), 16, 16 * 600, True
    if name in ("ba100", "ba100n"):   # LDS CSR, ragged rows: KV 4 at 128 columns, KV 2 at 64
        T = 128 if name == "ba100" else 64
        return G.barabasi_albert_metropolis(100, 2, seed=5), T, T * 600, True
    if name == "ring4200":   # LDS CSR, KV 8: nothing prefetched, no traced form
        e = [(i, (i + 1) % 4200) for i in range(4200)]
        return G.from_edge_weights(e, [0.25] * 4200, list(range(4200))), 4, 4 * 600, False
    e = G.torus_edges(64, 64)   # 4096 agents: 4-column tiles, KV 4, the lean traced form
    return G.from_edge_weights(e, [0.2] * len(e), list(range(4096))), 4, 4 * 600, True


CASES = [(g, lay) for g in ("reg1024", "ba100", "torus") for lay in ("tiled", "rows")] + \
        [(g, "tiled") for g in ("reg512", "ba100n", "ring4200")]


def coefs():
    from distributed_learning_amd.utils.fast_averaging import chebyshev_omegas
    return np.array([[np.float32(w), np.float32(1.0 - w)] for w in chebyshev_omegas(0.9, N_SEQ)],
                    np.float32)


def fold(csr, X):
    rp, col, w = csr.rowptr, csr.col, np.asarray(csr.w, X.dtype)
    out = np.empty_like(X)
    for a in range(len(rp) - 1):
        acc = np.zeros(X.shape[1], X.dtype)
        for e in range(rp[a], rp[a + 1]):
            acc = acc + w[e] * X[col[e]]
        out[a] = acc
    return out


@functools.lru_cache(maxsize=None)
def sequence(name, dtype=np.float32):
    csr, _, P, _ = graph(name)
    c = coefs().astype(dtype)
    u = [np.random.default_rng(11).standard_normal((csr.n_rows, P), dtype=np.float32).astype(dtype)]
    u.append(fold(csr, u[0]))
    for r in range(1, N_SEQ):
        u.append(c[r, 0] * fold(csr, u[r]) + c[r, 1] * u[r - 1])
    return u


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name,layout", CASES)
def test_passes_match_the_restatement(cuda, name, layout, K):
    from distributed_learning_amd import engine as eng
    u = sequence(name)
    csr, T, P, traced = graph(name)
    n, W = csr.n_rows, eng.DeviceCsr(csr, cuda)
    tiled = (P, T) if layout == "tiled" else None
    coef = torch.from_numpy(coefs().reshape(-1)).to(cuda)

    def put(A):
        t = torch.from_numpy(A).to(cuda)
        return eng.to_tiled(t, T) if tiled else t

    def same(t, want, what):
        got = (eng.from_tiled(t, P) if tiled else t).cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), what

    def run(X, Y, Z, Zout, first, dev=False):
        trace, dsq, dmax = (torch.zeros(k, device=cuda) for k in (K, n, 1))
        kw = dict(trace=trace if traced else None, dev_sq=dsq, dev_max=dmax) if dev else {}
        assert eng.cheb_rounds(W, X, Y, Z, Zout, coef[2 * first:], K, tiled=tiled, **kw) is True
        if dev:
            u64 = [v.astype(np.float64) for v in u[first + 1:first + K + 1]]
            want = [np.sqrt(((v - v.mean(0)) ** 2).sum(1)) for v in u64]
            tol = dict(rtol=DEV_RTOL, atol=dev_floor(u64[-1].mean(0), P))
            if traced:
                np.testing.assert_allclose(trace.cpu().numpy(), [w.max() for w in want], **tol)
            np.testing.assert_allclose(np.sqrt(dsq.cpu().numpy()), want[-1], **tol)
            np.testing.assert_allclose(dmax.item(), want[-1].max(), **tol)

    X, Y, Zo = put(u[0]), put(np.zeros_like(u[0])), put(np.zeros_like(u[0]))
    plan = eng.cheb_rounds_plan(W, X, Y, tiled=tiled)
    assert plan is not None and plan["n_tiles"] > plan["grid"], plan
    run(X, Y, None, Zo, 0, dev=True)   # a first pass: no z
    same(Y, u[K], "y of the first pass")
    same(Zo, u[K - 1], "z_out of the first pass")
    run(X, Y, None, None, 0)           # no outputs: the same bits
    same(Y, u[K], "y of the pass without outputs")
    for y_is_x in (True, False):   # K more rounds after SPLIT, in place (y = x or y = z)
        X, Z = put(u[SPLIT]), put(u[SPLIT - 1])
        run(X, X if y_is_x else Z, Z, Z if y_is_x else X, SPLIT, dev=True)
        same(X if y_is_x else Z, u[SPLIT + K], ("y", y_is_x))
        same(Z if y_is_x else X, u[SPLIT + K - 1], ("z_out", y_is_x))


@pytest.mark.parametrize("name", ["reg1024", "ba100", "torus", "reg512", "ring4200"])
def test_restatement_is_near_the_fp64_recurrence(name):
    deg, u32, u64 = np.diff(graph(name)[0].rowptr).max(), sequence(name), sequence(name, np.float64)
    for K in range(1, N_SEQ + 1):
        err = np.abs(u32[K] - u64[K]).max() / np.abs(u64[K]).max()
        assert err <= (deg + 3) * 2.0 ** -24 * K, (K, err)


@pytest.mark.parametrize("eps", [None, "inside a pass"])
def test_mix_chebyshev_in_passes_is_the_per_round_loop(cuda, eps):
    """eps=None: 11 rounds, one in-place pass; eps: the stop on round 11, inside the second pass."""
    from distributed_learning_amd import engine as E
    csr, T = graph("reg1024")[:2]
    n, P = csr.n_rows, 4 * T
    Wd = np.zeros((n, n))
    for a in range(n):
        Wd[a, csr.col[csr.rowptr[a]:csr.rowptr[a + 1]]] = csr.w[csr.rowptr[a]:csr.rowptr[a + 1]]
    gamma = float(np.abs(np.linalg.eigvalsh(Wd - 1.0 / n)).max())
    X0 = torch.from_numpy(np.random.default_rng(2).standard_normal((n, P), dtype=np.float32))

    def run(passes, eps, times):
        eng = E.GossipEngine(csr, P, device=cuda, X=X0.to(cuda), layout="tiled", tile_cols=T)
        devs = []
        done = eng.mix_chebyshev(gamma, times, eps, on_deviation=devs.append, passes=passes)
        return done, eng.rows().cpu().numpy(), devs

    if eps is None:
        ref, got = run(False, None, 11), run(True, None, 11)
    else:
        devs = run(False, 1e30, 11)[2]   # an eps every round meets: 11 evaluated rounds
        assert len(devs) == 11 and devs[10] < min(devs[:10])
        e = float(0.5 * (devs[10] + min(devs[:10])))
        ref, got = run(False, e, 1), run(True, e, 1)
    assert ref[0] == got[0] == 11
    assert np.array_equal(bits(got[1]), bits(ref[1]))
