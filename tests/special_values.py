"""Special-value inputs for the mixing kernels and the comparator the tests hold them to (TEST
INFRASTRUCTURE ONLY; plain numpy, no GPU).

Three classes of [n, P] fp32 matrices, standard_normal with special columns and one special row
written over them:

* ``tiny``: signed zeros, the smallest and the largest subnormal, 1e-40, the smallest normal, and
  6e-39 / 1e-30 whose product with a weight in (0, 1) is subnormal or underflows; every
  deviation stays finite.
* ``huge``: one-sign columns of |x| >= 2^127 (two or more of them overflow in any summation
  order, so a tree-summed and a row-order column mean agree on +-inf), a column where +3e38 and
  -3e38 meet in one row's neighbourhood, and for the stepped kernels a column where x - lr g
  overflows.  The special row alternates +-2^127, a lone huge entry per column, and no more:
  its mixed copies in a column (five of 0.2 * 1.5 * 2^127 in the Chebyshev test) sum below
  FLT_MAX.  With +-1.5 2^127 they do not: numpy's fp32 column sum overflows and its mean is inf
  where the true mean is 6e36 -- a class that depends on how a mean is summed, which these
  inputs are built to stay clear of.
* ``nonfinite``: one NaN element, a column with a single +inf, a column where +inf and -inf meet
  in one row (inf - inf), a column with a single -inf; ``zero_weight`` adds a CSR entry of weight
  exactly 0.0 pointing at the +inf (numpy: 0 * inf = NaN; a kernel skipping zero weights differs).

The special columns are spread over [0, P): the first at column 0, the last at P - 1 (the
guarded tail of an unaligned width).  Where P has fewer columns than the class has features the
first P features are kept, so a P = 1 shape carries one feature and cannot meet every condition
of tests/test_special_values_cpu.py (which says so).
"""
import dataclasses
from collections import namedtuple

import numpy as np

from oracle import cref

CLASSES = ("tiny", "huge", "nonfinite")
LR = 0.05

F = np.float32
MIN_SUB = np.uint32(0x00000001).view(F)     # 2^-149
MAX_SUB = np.uint32(0x007FFFFF).view(F)
MIN_NORM = np.uint32(0x00800000).view(F)    # 2^-126
TINY = np.array([MAX_SUB, -0.0, 1e-40, 0.0, MIN_SUB, -MIN_SUB, -1e-40, -MAX_SUB, MIN_NORM,
                 -MIN_NORM, 6e-39, -6e-39, 1e-30, -1e-30], F)
P127 = F(2.0 ** 127)

Case = namedtuple("Case", "X G lr csr")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def mismatches(got, want):
    """Boolean mask of the elements ``same_bits`` rejects."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    if got.shape != want.shape:
        raise AssertionError(f"shapes differ: {got.shape} against {want.shape}")
    nan = np.isnan(want)
    return np.where(nan, ~np.isnan(got), bits(got) != bits(want))


def same_bits(got, want):
    """Where ``want`` is not NaN the uint32 bits are equal (the sign of zero, subnormals and the
    sign of infinities included); where it is NaN ``got`` is NaN, sign and payload not compared."""
    return not mismatches(got, want).any()


def describe(got, want, limit=6):
    """The first mismatches as text, for an assertion message."""
    bad = np.argwhere(mismatches(got, want))
    got, want = np.asarray(got, F), np.asarray(want, F)
    items = [f"{tuple(int(v) for v in i)}: got {got[tuple(i)]!r} want {want[tuple(i)]!r}"
             for i in bad[:limit]]
    return f"{len(bad)} of {want.size} elements differ; " + "; ".join(items)


def feature_columns(P, k):
    """Column of each of k features (None where P has no column left for it): spread evenly,
    feature 0 at column 0, feature k - 1 at column P - 1."""
    out, used = [], set()
    for i in range(k):
        c = (i * (P - 1)) // max(k - 1, 1)
        if c in used:
            out.append(None)
        else:
            used.add(c)
            out.append(c)
    return out


def _pair_in_one_row(csr):
    """(a, b): two different source agents (below n_rows) that one row mixes -- the pair whose
    columns of W have the smallest absolute sums: +-3e38 at a and b then leaves outputs w * 3e38
    whose one-sign total stays below FLT_MAX where that sum is below 1.1, so the output's column
    mean does not overflow in one summation order and not in another."""
    n = len(csr.rowptr) - 1
    load = np.bincount(csr.col, weights=np.abs(csr.w), minlength=n)
    best = None
    for q in range(n):
        nb = []
        for c in csr.col[csr.rowptr[q]:csr.rowptr[q + 1]]:
            if int(c) < n and int(c) not in nb:
                nb.append(int(c))
        nb.sort(key=lambda c: load[c])
        if len(nb) >= 2 and (best is None or load[nb[1]] < best[0]):
            best = (load[nb[1]], nb[0], nb[1])
    if best is None:
        raise ValueError("no row mixes two different agents")
    return best[1], best[2]


def zero_weight(csr, src):
    """csr with one entry that points at source agent ``src`` (off the diagonal where there is
    one) given the weight exactly 0.0."""
    n = len(csr.rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(csr.rowptr))
    hit = np.flatnonzero(csr.col == src)
    off = [e for e in hit if rows[e] != src]
    if not len(hit):
        raise ValueError(f"no entry points at agent {src}")
    w = np.array(csr.w, np.float64)
    w[off[0] if off else hit[0]] = 0.0
    return dataclasses.replace(csr, w=w)


def inf_agent(csr):
    """The agent that holds the single +inf of the ``nonfinite`` class."""
    return (len(csr.rowptr) - 1) // 2


def build(cls, n, P, csr, seed=0, zero=False):
    """Case(X, G, lr, csr) of a class on csr's graph (n == csr.n_rows).  X alone feeds the plain
    kernels; (X, G, lr) the stepped ones.  zero (``nonfinite`` only): the returned csr has a
    0.0-weight entry at the +inf agent."""
    assert cls in CLASSES and n == len(csr.rowptr) - 1
    rng = np.random.default_rng(1000 * CLASSES.index(cls) + seed)
    X = rng.standard_normal((n, P), dtype=F)
    G = rng.standard_normal((n, P), dtype=F)
    r = np.arange(n)
    r0 = 1 % n                       # the special row
    a, b = _pair_in_one_row(csr) if n > 1 else (0, 0)
    if cls == "tiny":
        p = np.arange(P)
        X[r0] = TINY[p % len(TINY)]
        G[r0] = TINY[(p + 3) % len(TINY)]
        for j, c in enumerate(feature_columns(P, 5)):
            if c is None:
                continue
            X[:, c] = TINY[(r * (j + 1) + j) % len(TINY)]
            G[:, c] = TINY[(r * 3 + j + 5) % len(TINY)]
            if j == 1:               # -0.0 - lr * +0.0 = -0.0: the stepped kernels keep the sign
                X[:, c] = -0.0
                G[:, c] = 0.0
    elif cls == "huge":
        ramp = P127 * (F(1.25) + F(0.5) * ((r * 5) % 8).astype(F) / F(8))   # [1.25, 1.75) 2^127
        p = np.arange(P)
        X[r0] = np.where(p % 2 == 0, F(1.0), F(-1.0)) * P127
        cols = feature_columns(P, 4)
        if cols[0] is not None:
            X[:, cols[0]] = ramp
        if cols[1] is not None:      # x - lr g overflows at two agents, both to +inf
            c = cols[1]
            X[r0, c] = G[r0, c]      # (an ordinary value again)
            for q in (a, b):
                X[q, c] = 3.39e38
                G[q, c] = -3.4e38
        if cols[2] is not None:      # +3e38 and -3e38 in one row's neighbourhood
            c = cols[2]
            X[r0, c] = G[r0, c]
            X[a, c], X[b, c] = 3e38, -3e38
        if cols[3] is not None:
            X[:, cols[3]] = -ramp
    else:
        h = inf_agent(csr)
        cols = feature_columns(P, 4)
        if cols[0] is not None:
            X[(n - 1) // 3, cols[0]] = np.nan
            if n > 4:                              # stepped: inf - lr inf = NaN here as well
                e = (n - 1) // 3 + 1
                X[e, cols[0]] = G[e, cols[0]] = np.inf
        if cols[1] is not None:
            X[h, cols[1]] = np.inf
            G[h, cols[1]] = -np.inf                # inf + lr inf = inf
        if cols[2] is not None:
            X[a, cols[2]], X[b, cols[2]] = np.inf, -np.inf
        if cols[3] is not None:
            X[n - 1, cols[3]] = -np.inf
            G[(n - 1) // 2, cols[3]] = np.inf      # x - lr inf = -inf from a finite x
        if zero:
            csr = zero_weight(csr, h)
    return Case(X, G, LR, csr)


# ---------------------------------------------------------------- the shapes the GPU tests run
def _golden_csr(tag):
    import os
    from distributed_learning_amd.graph import Csr
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                             "mix_rr4_n64.npz"))
    return Csr(d[f"{tag}_rowptr"], d[f"{tag}_cols"], d[f"{tag}_w"])


def _random_csr(n, deg, seed, cls, uniform=False):
    """test_mix_gpu.graph_csr: random directed neighbours.  Its random weights lie in
    (-0.3, 0.9); a one-sign huge column mixed with them leaves +-1e38 outputs of both signs,
    whose column sum overflows in one summation order and not in another.  The ``huge`` class
    therefore takes the builder's uniform weights (1 / row length): every output of a one-sign
    huge column is again >= 2^127 of that sign."""
    from test_mix_gpu import graph_csr
    return graph_csr(n, deg, seed=seed,
                     weights="uniform" if uniform or cls == "huge" else "random")


def _circulant(n):
    from cheb_oracle import circulant_csr
    return circulant_csr(n)


def _rr(n, seed):
    from test_mix_trace_gpu import rr_csr
    return rr_csr(n, seed)


def _metro():
    from test_mix_trace_gpu import metropolis_csr
    return metropolis_csr(50, 0.1, 2)


# name: (graph builder of the class, n, P, zero-weight entry in the nonfinite class).  The zero
# weight goes only into graphs that are not doubly stochastic to begin with: it would take a
# doubly stochastic graph off the kernel the case is named for.
SHAPES = {
    "small_8x37": (lambda c: _random_csr(8, 3, 8, c), 8, 37, True),
    "rows_64x256": (lambda c: _random_csr(64, 4, 64, c), 64, 256, True),
    "gather_64x1000": (lambda c: _random_csr(64, 5, 64, c), 64, 1000, True),
    "reg4_64x64": (lambda c: _golden_csr("a"), 64, 64, False),
    "reg5_64x64": (lambda c: _golden_csr("b"), 64, 64, False),
    "halo_40x70": (lambda c: _random_csr(40, 4, 3, c), 40, 70, True),
    "rounds_64x4096": (lambda c: _random_csr(64, 4, 64, c), 64, 4096, True),
    "rounds_100x1024": (lambda c: _random_csr(100, 5, 100, c), 100, 1024, True),
    "rounds_rr64x256": (lambda c: _rr(64, 1), 64, 256, False),
    "trace_rr300x256": (lambda c: _rr(300, 7), 300, 256, False),
    "trace_metro50x1000": (lambda c: _metro(), 50, 1000, False),
    "until_5x617": (lambda c: _random_csr(5, 3, 1, c, uniform=True), 5, 617, False),
    "until_16x63": (lambda c: _random_csr(16, 3, 3, c, uniform=True), 16, 63, False),
    "until_3x1": (lambda c: _random_csr(3, 2, 4, c, uniform=True), 3, 1, False),
    "fused_33x129": (lambda c: _random_csr(33, 4, 33 + 129, c), 33, 129, True),
    "fused_circ64x256": (lambda c: _circulant(64), 64, 256, False),
}


def shape_case(name, cls):
    """The Case of a named shape and class."""
    graph, n, P, zero = SHAPES[name]
    return build(cls, n, P, graph(cls), seed=len(name), zero=zero)


def dev_sq32(Y, mean=None):
    """The oracle's per-agent squared deviation (cref.deviation_sq, fp64 sums about numpy's
    row-order fp32 mean) as the fp32 value the device reports: above FLT_MAX it is inf."""
    with np.errstate(all="ignore"):
        return cref.deviation_sq(Y, mean).astype(F)


def dev_max32(Y, mean=None):
    """np.max(np.sqrt(dev_sq)): NaN when any agent's deviation is NaN, else inf when one is."""
    with np.errstate(all="ignore"):
        return np.max(np.sqrt(dev_sq32(Y, mean)))


def classes_of(v):
    """0 finite, 1 +inf, 2 -inf, 3 NaN, elementwise."""
    v = np.asarray(v, np.float64)
    return np.where(np.isnan(v), 3, np.where(np.isposinf(v), 1, np.where(np.isneginf(v), 2, 0)))
