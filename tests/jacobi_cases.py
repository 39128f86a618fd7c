"""Inputs of the direct c1-kernel tests (test_perron_direct_gpu.py, test_async_update_gpu.py,
test_consensus_gd_gpu.py) and their oracle results, computed once per process and shared.
test_jacobi_oracle_cpu.py checks on the CPU that none of them sits on a knife edge: every
convergence test of every iteration is at least 1e-6 relative away from its conv_eps."""
import functools
import zlib

import numpy as np

import jacobi_oracle as O

K_LDS_BYTES = 163840          # dl::kLdsBytes (csrc/dl_internal.h): the planner's LDS budget
MARGIN = 1e-6
DTYPES = {"f64": np.float64, "f32": np.float32}


def perron_tile_cols(dtype, n_rows, n_params):
    """perron_tile_cols of csrc/aux_kernels.hip: n_params when both ping-pong buffers fit one
    workgroup's LDS (single launch), else the column-tile width of the host-iterated path
    (0: not even one column fits)."""
    sz = np.dtype(dtype).itemsize
    if 2 * n_rows * n_params * sz + 16 <= K_LDS_BYTES:
        return n_params
    return max(0, min(1024, (K_LDS_BYTES - 16) // (n_rows * sz)))


def single_limit(dtype, n_rows):
    """Widest n_params that still runs as one launch."""
    return (K_LDS_BYTES - 16) // (2 * n_rows * np.dtype(dtype).itemsize)


# ------------------------------------------------------------------ dl_perron_round
def _ring8():
    return O.csr_from_edges(O.GRAPHS["ring8"])[1:]


def _torus():
    return O.csr_from_edges(O.GRAPHS["torus8x8"])[1:]


def _isolated():
    """Ring over agents 0 1 2 4 5 6 7; agent 3 has no neighbours (rowptr[3] == rowptr[4])."""
    ring = [0, 1, 2, 4, 5, 6, 7]
    rowptr, col = [0], []
    for a in range(8):
        if a in ring:
            i = ring.index(a)
            col += [ring[i - 1], ring[(i + 1) % 7]]
        rowptr.append(len(col))
    return np.asarray(rowptr, np.int32), np.asarray(col, np.int32)


def _special(Y, kind, rowptr, col):
    """Plant the special values of one case into standard-normal Y."""
    n, P = Y.shape
    if kind == "negzero":
        Y[:, 1] = -0.0                       # a whole column of -0.0
        r = 5                                # and one agent whose neighbourhood alone holds it
        Y[[r] + list(col[rowptr[r]:rowptr[r + 1]]), P - 2] = -0.0
    elif kind == "nan":
        Y[2, P // 2] = np.nan
    elif kind == "inf":
        Y[1, 0] = np.inf
        Y[n - 1, P - 1] = -np.inf
        Y[3, 2], Y[4, 2] = np.inf, -np.inf    # neighbours: inf - inf, a NaN in the first sum
    return Y


# name: graph, P (a width, or one the dtype decides: the single-launch limit, one past it, the
# three-tile width MULTI_P) and
#   weights: integer weights 1..n;  pad: ldy - P;
#   k: the round stops at iteration k, at a conv_eps taken from the oracle's own gaps;
#   cut: conv_eps = 0 and max_iter = cut;
#   strict: (row, k_loose, k) per-agent conv_eps, every agent at iteration k_loose's value but
#   one, which asks for iteration k's and so decides the count;
#   special: planted values; conv / max_iter: given as they stand
PERRON_CASES = {
    "ring8": dict(graph=_ring8, P=33, k=6),
    "ring8_w_pad": dict(graph=_ring8, P=33, weights=True, pad=5, k=7),
    "ring8_conv_rows": dict(graph=_ring8, P=33, weights=True, pad=5, strict=(3, 4, 9)),
    "isolated": dict(graph=_isolated, P=33, weights=True, k=6),
    "cut1": dict(graph=_ring8, P=33, weights=True, cut=1),
    "cut2": dict(graph=_ring8, P=33, weights=True, cut=2),
    "cut3": dict(graph=_ring8, P=33, weights=True, cut=3),
    "single_limit": dict(graph=_torus, P="limit", weights=True, k=5),
    "past_limit": dict(graph=_torus, P="limit+1", weights=True, pad=3, k=5),
    "multi_odd": dict(graph=_torus, P="multi", weights=True, pad=3, cut=3),
    "multi_even": dict(graph=_torus, P="multi", weights=True, pad=3, cut=4),
    "multi_conv": dict(graph=_torus, P="multi", weights=True, pad=3, k=6),
    "multi_conv_rows": dict(graph=_torus, P="multi", pad=3, strict=(17, 3, 7)),
    "negzero_single": dict(graph=_ring8, P=33, special="negzero", cut=1),
    "negzero_single_w": dict(graph=_ring8, P=33, weights=True, special="negzero", cut=3),
    "negzero_multi": dict(graph=_torus, P="multi", weights=True, special="negzero", cut=2),
    "nan_single": dict(graph=_ring8, P=33, special="nan", conv=1e-3, max_iter=4),
    "nan_multi": dict(graph=_torus, P="multi", pad=3, special="nan", conv=1e-3, max_iter=4),
    "inf_single": dict(graph=_ring8, P=33, special="inf", conv=1e-3, max_iter=4),
    "inf_multi": dict(graph=_torus, P="multi", special="inf", conv=1e-3, max_iter=3),
}
MULTI_P = {"f64": 700, "f32": 1300}


@functools.lru_cache(maxsize=None)
def perron_case(name, dt):
    """One case's inputs and oracle result: dict with Y0 [n, P], rowptr, col, eps, conv_eps,
    conv_rows, weight, mean_w, max_iter, pad, want (Y, k), trace."""
    spec, dtype = PERRON_CASES[name], DTYPES[dt]
    rowptr, col = spec["graph"]()
    n = len(rowptr) - 1
    P = spec["P"]
    if P == "limit":
        P = single_limit(dtype, n)
    elif P == "limit+1":
        P = single_limit(dtype, n) + 1
    elif P == "multi":
        P = MULTI_P[dt]
    rng = np.random.default_rng(zlib.crc32(f"{name}/{dt}".encode()))
    Y0 = rng.standard_normal((n, P)).astype(dtype)
    if "special" in spec:
        Y0 = _special(Y0, spec["special"], rowptr, col)
    eps = O.max_degree_eps(rowptr)
    weight = [float(w) for w in range(1, n + 1)] if spec.get("weights") else None
    mean_w = (n + 1) / 2 if weight else 1.0
    c = dict(Y0=Y0, rowptr=rowptr, col=col, eps=eps, weight=weight, mean_w=mean_w,
             pad=spec.get("pad", 0), conv_rows=None, P=P, n=n, dtype=dtype)
    run = functools.partial(O.jacobi_round, Y0, rowptr, col, eps, weight=weight, mean_w=mean_w)
    if "cut" in spec:
        c["conv_eps"], c["max_iter"] = 0.0, spec["cut"]
    elif "conv" in spec:
        c["conv_eps"], c["max_iter"] = spec["conv"], spec["max_iter"]
    else:
        free = []
        run(conv_eps=-1.0, max_iter=12, trace=free)      # never converges: the gaps alone
        if "k" in spec:
            c["conv_eps"], c["max_iter"] = O.conv_between(free, spec["k"]), 32
        else:
            # every agent but one stops at k_loose; that one asks for the global k's conv_eps
            row, k_loose, k = spec["strict"]
            rows = [O.conv_between(free, k_loose)] * n
            rows[row] = O.conv_between(free, k)
            c["conv_eps"], c["conv_rows"], c["max_iter"] = 123.0, rows, 32
            c["k_loose"] = k_loose
    c["trace"] = []
    c["want"] = run(conv_eps=c["conv_eps"], conv_rows=c["conv_rows"], max_iter=c["max_iter"],
                    trace=c["trace"])
    return c


# the row limit: one fp64 column of 20478 agents fills the LDS tile (TP == 1)
ROW_LIMIT = (K_LDS_BYTES - 16) // 8


@functools.lru_cache(maxsize=None)
def row_limit_case():
    rowptr, col = O.ring_csr(ROW_LIMIT)
    Y0 = np.random.default_rng(77).standard_normal((ROW_LIMIT, 3))
    eps = O.max_degree_eps(rowptr)
    want = O.jacobi_round(Y0, rowptr, col, eps, conv_eps=0.0, max_iter=2)
    return dict(Y0=Y0, rowptr=rowptr, col=col, eps=eps, want=want)


# ------------------------------------------------------------------ dl_async_update
ASYNC_D = [0, 1, 7, 8, 9, 15, 16, 17, 24, 63, 64]


def async_scalars(d, f32):
    """d + 1 values of mixed magnitudes (own value first): full fp64 draws, or fp32-representable
    ones for the sum_f32 path (whose neighbours are fp32 pre-scaled values)."""
    rng = np.random.default_rng(500 + 97 * d)
    v = rng.standard_normal(d + 1) * 10.0 ** rng.uniform(-3, 3, d + 1)
    return v.astype(np.float32).astype(np.float64) if f32 else v


def async_vectors(n, d, f32):
    """[d + 1, n] values (own first) of mixed magnitudes, as async_scalars."""
    rng = np.random.default_rng(900 + 13 * d)
    v = rng.standard_normal((d + 1, n)) * 10.0 ** rng.uniform(-3, 3, (d + 1, n))
    return v.astype(np.float32).astype(np.float64) if f32 else v


# ------------------------------------------------------------------ dl_consensus_gd
def _graph_ring_plus_isolated():
    """Ring over agents 0 1 3 4 5; agent 2 has no neighbours."""
    ring = [0, 1, 3, 4, 5]
    rowptr, col = [0], []
    for a in range(6):
        if a in ring:
            i = ring.index(a)
            col += [ring[i - 1], ring[(i + 1) % 5]]
        rowptr.append(len(col))
    return np.asarray(rowptr, np.int32), np.asarray(col, np.int32)


SIZES12 = [1, 2, 63, 64, 65, 3, 127, 128, 129, 17, 90, 200]
GD_CASES = {
    # name: graph, features, shard sizes, conv_eps (None: 0 with max_iter as a cut), max_iter
    "crosscheck": dict(graph=lambda: O.csr_from_edges(O.ring_edges(12))[1:], F=5, sizes=SIZES12,
                       conv=2e-2, max_iter=64, iters=3, zero_steps=True),
    "a_ring12_f16": dict(graph=lambda: O.csr_from_edges(O.ring_edges(12))[1:], F=16,
                         sizes=SIZES12, conv=2e-2, max_iter=64, iters=10),
    "b_torus20_f1": dict(graph=lambda: O.csr_from_edges(O.torus_edges(4, 5))[1:], F=1,
                         sizes=[5, 1, 64, 30, 2, 65, 7, 63, 10, 33, 12, 70, 3, 20, 100, 9, 41, 8,
                                66, 11], conv=2e-2, max_iter=64, iters=10),
    "c_global_f16": dict(graph=lambda: O.csr_from_edges(O.GRAPHS["k4"])[1:], F=16,
                         sizes=[1, 65, 634, 700], conv=1e-3, max_iter=64, iters=10),
    "d_isolated": dict(graph=_graph_ring_plus_isolated, F=7, sizes=[30, 1, 40, 64, 65, 40],
                       conv=1e-2, max_iter=64, iters=10),
    "e_cut2": dict(graph=lambda: O.csr_from_edges(O.ring_edges(12))[1:], F=16, sizes=SIZES12,
                   conv=0.0, max_iter=2, iters=10),
}


def gd_lds_bytes(n_agents, n_features, rows, x_in_lds):
    """gd_lds_bytes of csrc/consensus_gd.hip."""
    off = (3 * n_agents * n_features * 8 + 4 + 15) // 16 * 16
    return off + (rows * n_features * 8 + rows * 8 if x_in_lds else 0)


@functools.lru_cache(maxsize=None)
def gd_case(name):
    spec = GD_CASES[name]
    rowptr, col = spec["graph"]()
    R, F = len(rowptr) - 1, spec["F"]
    assert R == len(spec["sizes"])
    sp = np.concatenate([[0], np.cumsum(spec["sizes"])]).astype(np.int32)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    X = rng.standard_normal((int(sp[-1]), F))
    y = rng.choice([-1.0, 1.0], int(sp[-1]))
    W0 = 0.5 * rng.standard_normal((R, F))
    T = spec["iters"]
    steps = np.zeros(T) if spec.get("zero_steps") else 0.1 * np.arange(1, T + 1) ** -0.5
    return dict(X=X, y=y, sp=sp, W0=W0, rowptr=rowptr, col=col, eps=O.max_degree_eps(rowptr),
                conv_eps=spec["conv"], steps=steps, tau=1e-4, max_iter=spec["max_iter"], R=R,
                F=F)


@functools.lru_cache(maxsize=None)
def gd_want(name, longdouble=False):
    """(W, ks, trace) of the oracle; longdouble: the gradient's dot products in np.longdouble."""
    c, trace = gd_case(name), []
    W, ks = O.consensus_gd(c["X"], c["y"], c["sp"], c["W0"], c["rowptr"], c["col"], c["eps"],
                           c["conv_eps"], c["steps"], c["tau"], c["max_iter"],
                           gradient=O.logreg_gradient_ld if longdouble else
                           O.M.logreg_gradient, trace=trace)
    return W, ks, trace
