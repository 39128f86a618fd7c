"""Plain-numpy oracle of the three fp64 / fp32 kernels behind BASELINE config c1 (TEST
INFRASTRUCTURE ONLY): ``dl_perron_round``, ``dl_async_load`` / ``dl_async_update`` and
``dl_consensus_gd``.  Every function is the reference's own numpy expression
(utils/consensus_asyncio.py:231, :295, :297) on CSR adjacency, in the dtype of the values it is
given; tests/test_jacobi_oracle_cpu.py ties it bit for bit to oracle/mixer_ref.jacobi_round,
which is pinned to the reference's runs.

fp32: the scalars (``eps``, ``conv_eps``, ``weight``, ``mean_w``) must be PYTHON floats.  Under
NEP 50 a Python float next to a float32 array is cast to float32 first, which is exactly the
``(DT)`` casts of ``perron_update`` / ``prescale`` in csrc/aux_kernels.hip; a numpy float64 scalar
would promote the expression to float64 instead.  Every entry point therefore passes its scalars
through ``float()``.
"""
import numpy as np

from oracle import mixer_ref as M


# ------------------------------------------------------------------ graphs
def csr_from_edges(edges):
    """(tokens, rowptr, col) of an edge list: agents in ``ConsensusNetwork.tokens`` order,
    neighbours in socket order (mixer_ref.asyncio_tokens / asyncio_neighbors)."""
    edges = [tuple(e) for e in edges]
    tokens = M.asyncio_tokens(edges)
    index = {t: i for i, t in enumerate(tokens)}
    rowptr, col = [0], []
    for t in tokens:
        col.extend(index[j] for j in M.asyncio_neighbors(edges, t))
        rowptr.append(len(col))
    return tokens, np.asarray(rowptr, np.int32), np.asarray(col, np.int32)


def ring_csr(n):
    """Ring of n agents, neighbours of r in the order (r - 1, r + 1) mod n (no edge list: the
    row-limit case has 20478 agents)."""
    r = np.arange(n)
    col = np.stack([(r - 1) % n, (r + 1) % n], axis=1).reshape(-1)
    return np.arange(0, 2 * n + 1, 2, dtype=np.int32), col.astype(np.int32)


def ring_edges(n):
    return [(i, (i + 1) % n) for i in range(n)]


def torus_edges(rows, cols):
    edges = []
    for r in range(rows):
        for c in range(cols):
            a = r * cols + c
            edges.append((a, r * cols + (c + 1) % cols))
            edges.append((a, ((r + 1) % rows) * cols + c))
    return edges


GRAPHS = {
    "ring8": ring_edges(8),
    "k4": [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)],
    "grid5": [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4), (1, 3)],
    "star9": [(0, i) for i in range(1, 9)],
    "torus8x8": torus_edges(8, 8),
}


def max_degree_eps(rowptr):
    """``ConsensusNetwork.__calc_eps`` (:78-86): 0.95 / max degree, as a Python float."""
    return float(0.95 / np.max(np.diff(rowptr)))


# ------------------------------------------------------------------ dl_perron_round
def prescale(v, weight, mean_w):
    """``y = v * weight / mean_w`` (:231) in v's dtype."""
    return v * float(weight) / float(mean_w)


def jacobi_step(Y, rowptr, col, eps, conv_eps=None, conv_rows=None):
    """One synchronous iteration over all agents: ``y*(1 - eps*deg) + eps*np.sum(nbrs, axis=0)``
    (:295; 0.0 for an agent without neighbours) and the one-sided test against the neighbours'
    previous values (:297).  Returns (Y', any agent's test failed)."""
    eps = float(eps)
    new = np.empty_like(Y)
    any_fail = False
    for r in range(len(rowptr) - 1):
        nv = [Y[c] for c in col[rowptr[r]:rowptr[r + 1]]]
        s = np.sum(nv, axis=0) if nv else 0.0
        ce = float(conv_eps if conv_rows is None else conv_rows[r])
        with np.errstate(invalid="ignore"):      # inf - inf: a NaN, which fails the test
            new[r] = Y[r] * (1 - eps * len(nv)) + eps * s
            if not all(np.all((new[r] - v) <= ce) for v in nv):
                any_fail = True
    return new, any_fail


def jacobi_round(Y, rowptr, col, eps, conv_eps=None, weight=None, mean_w=1.0, conv_rows=None,
                 max_iter=64, trace=None):
    """Pre-scale (when ``weight`` is given), then iterate until no agent's test fails or
    ``max_iter``.  Returns (Y, k).  ``trace``: a list that receives, per iteration, the per-agent
    largest ``y' - v`` (``row_gaps``)."""
    Y = np.array(Y)
    if weight is not None:
        Y = np.stack([prescale(Y[r], weight[r], mean_w) for r in range(Y.shape[0])])
    for k in range(1, int(max_iter) + 1):
        new, fail = jacobi_step(Y, rowptr, col, eps, conv_eps, conv_rows)
        if trace is not None:
            trace.append(row_gaps(Y, new, rowptr, col))
        Y = new
        if not fail:
            return Y, k
    return Y, int(max_iter)


def row_gaps(Y, new, rowptr, col):
    """Per agent, the largest ``y' - v`` over its neighbours and coordinates, in Y's dtype
    (-inf for an agent without neighbours): what the convergence test compares with conv_eps."""
    g = np.full(len(rowptr) - 1, -np.inf)
    for r in range(len(rowptr) - 1):
        for c in col[rowptr[r]:rowptr[r + 1]]:
            with np.errstate(invalid="ignore"):
                g[r] = max(g[r], float(np.max(new[r] - Y[c])))
    return g


def conv_between(trace, k):
    """A conv_eps at which the round stops at iteration k: half-way between the largest gap of
    iteration k and the smallest largest-gap of the iterations before it."""
    top = [float(np.max(g)) for g in trace]
    assert 1 < k <= len(top) and top[k - 1] < min(top[:k - 1]), top
    return 0.5 * (top[k - 1] + min(top[:k - 1]))


def margin(trace, conv_eps=None, conv_rows=None):
    """Smallest relative distance of any agent's largest gap, at any iteration, from the conv_eps
    it is compared with.  A test whose margin is >= 1e-6 cannot flip on a last-place difference."""
    conv = np.full(len(trace[0]), float(conv_eps)) if conv_rows is None else \
        np.asarray(conv_rows, np.float64)
    assert np.all(conv != 0)
    worst = np.inf
    for g in trace:
        fin = np.isfinite(g)
        worst = min(worst, float(np.min(np.abs(g[fin] - conv[fin]) / np.abs(conv[fin]))))
    return worst


# ------------------------------------------------------------------ dl_async_*
def async_load(v, weight, mean_w, mode):
    """``value * weight / mean_weight`` (:231): mode 0 in fp64, mode 1 in fp32 (an fp32 value
    with weak Python scalars).  Returned as float64 (the arena's type)."""
    v = np.asarray(v, np.float32 if mode == 1 else np.float64)
    return (v * float(weight) / float(mean_w)).astype(np.float64)


def async_update(y, nbrs, keep, eps, conv_eps, f32_sum):
    """One agent step (:295, :297): ``y*keep + eps*np.sum(nbrs, axis=0)`` with numpy float64
    ``keep`` and ``eps`` (the reference's eps is a numpy scalar) and the verdict
    ``all((y' - v) <= conv_eps)``.  ``f32_sum``: the neighbours' values are fp32 arrays (all of
    them fp32 pre-scaled values), so numpy sums them in fp32.  Values are 0-d (the (d,) stack is
    reduced along its contiguous axis, pairwise) or (P,) arrays."""
    vals = [np.asarray(v, np.float32) for v in nbrs] if f32_sum else list(nbrs)
    s = np.sum(vals, axis=0) if vals else 0.0
    new = y * np.float64(keep) + np.float64(eps) * s
    assert np.asarray(new).dtype == np.float64
    return new, all(bool(np.all((new - v) <= conv_eps)) for v in nbrs)


def left_fold(vals):
    """Sequential sum from +0.0 (what a pairwise reduction must differ from for some d >= 8)."""
    s = np.float64(0.0) if np.asarray(vals[0]).dtype == np.float64 else np.float32(0.0)
    for v in vals:
        s = s + v
    return s


# ------------------------------------------------------------------ dl_consensus_gd
def logreg_step(Xs, ys, w, step, tau, gradient=M.logreg_gradient):
    """Local GD step ``w - step * gradient`` on one shard (notebook cell 13)."""
    return w - step * gradient(Xs, ys, w, tau)


def logreg_gradient_ld(X, y, w, tau=1e-4):
    """mixer_ref.logreg_gradient with ``X @ w`` and the per-feature dot products accumulated in
    np.longdouble (rounded to fp64 once): measures what the fp64 oracle's own summation costs."""
    Xl, yl = X.astype(np.longdouble), y.astype(np.longdouble)
    z = np.asarray((Xl * w.astype(np.longdouble)).sum(axis=1), np.float64)
    c = (y * (1.0 / (1.0 + np.exp(-(-y * z))))).astype(np.longdouble)
    dots = np.array([float((c * Xl[:, j]).sum()) for j in range(X.shape[1])])
    return -dots / X.shape[0] + tau * w


def consensus_gd(X, y, shard_ptr, W0, rowptr, col, eps, conv_eps, steps, tau, max_iter,
                 gradient=M.logreg_gradient, trace=None):
    """dl_consensus_gd: per iteration a local step of every agent on its shard, then one Jacobi
    round weighted by the shard sizes.  Returns (W, [Jacobi iterations per round])."""
    W = np.array(W0, np.float64)
    sizes = [int(n) for n in np.diff(shard_ptr)]
    mean_w = sum(sizes) / len(sizes)
    ks = []
    for step in steps:
        W = np.stack([logreg_step(X[shard_ptr[a]:shard_ptr[a + 1]],
                                  y[shard_ptr[a]:shard_ptr[a + 1]], W[a], float(step), tau,
                                  gradient) for a in range(len(sizes))])
        W, k = jacobi_round(W, rowptr, col, eps, conv_eps, weight=sizes, mean_w=mean_w,
                            max_iter=max_iter, trace=trace)
        ks.append(k)
    return W, ks


def same_bits(got, want):
    """Bit equality that lets NaN payloads differ: NaNs in the same places, every other element
    (signed zeros and infinities included) the same bits."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(got.view(u)[~nan], want.view(u)[~nan]))
