"""numpy restatement of the Chebyshev-accelerated gossip loop (GossipEngine.mix_chebyshev), shared
by test_chebyshev_host.py and test_cheb_round_gpu.py.  The fold is the oracle's (cref.mix_round,
bit for bit Mixer._mix_params_once), the combination the rule of include/dlamd.h:
y = float32(a) * ACC + float32(b) * Z, three separately rounded fp32 operations.  Deviations are
taken about an fp64 mean, in fp64: the reference the device's fp32 values are held against."""
import functools

import numpy as np

from oracle import cref


def circulant_csr(n):
    """The tests' circulant graph of degree 4 with one uniform weight (test_sgd_round_gpu's
    regular_csr): symmetric, so doubly stochastic."""
    from distributed_learning_amd.graph import Csr
    cl = np.concatenate([[a, (a + 1) % n, (a - 1) % n, (a + 2) % n, (a - 2) % n]
                         for a in range(n)])
    return Csr(np.arange(0, 5 * n + 1, 5), cl, np.full(cl.size, 0.2))


def spectral_radius(csr):
    """gamma: the spectral radius of W - 11^T/n (W symmetric), from the fp32 weights."""
    W = np.zeros((csr.n_rows, csr.n_rows))
    rows = np.repeat(np.arange(csr.n_rows), np.diff(csr.rowptr))
    np.add.at(W, (rows, csr.col), csr.w.astype(np.float32).astype(np.float64))
    assert np.array_equal(W, W.T)
    return float(np.max(np.abs(np.linalg.eigvalsh(W - 1.0 / csr.n_rows))))


def cheb_step(acc, Z, a, b):
    """The round's second line on the folded ACC = W x and the previous iterate Z."""
    return np.float32(a) * acc + np.float32(b) * Z


def max_deviation(X):
    """max_a ||x_a - mean|| in fp64 about the fp64 column mean."""
    X64 = X.astype(np.float64)
    return float(np.sqrt(((X64 - X64.mean(axis=0)) ** 2).sum(axis=1).max()))


def plain_rounds(csr, X0, rounds):
    """[(X, max deviation) after round 1..rounds] of X <- W X."""
    out, X = [], X0
    for _ in range(rounds):
        X = cref.mix_round(X, csr.rowptr, csr.col, csr.w)
        out.append((X, max_deviation(X)))
    return out


def cheb_rounds(csr, X0, gamma, rounds):
    """[(X, max deviation) after round 1..rounds] of the Chebyshev semi-iteration: round 1 the
    plain round, round k the fold of x_{k-1} combined with x_{k-2}."""
    from distributed_learning_amd.utils.fast_averaging import chebyshev_omegas
    om = chebyshev_omegas(gamma, rounds)
    out, prev, X = [], None, X0
    for k in range(rounds):
        acc = cref.mix_round(X, csr.rowptr, csr.col, csr.w)
        new = acc if k == 0 else cheb_step(acc, prev, om[k], 1.0 - om[k])
        prev, X = X, new
        out.append((X, max_deviation(X)))
    return out


def rounds_until(devs, eps, times=1):
    """The reference's stop rule over a deviation sequence: the first round k >= times (1-based)
    with devs[k - 1] < eps, or None."""
    for k, d in enumerate(devs, 1):
        if d < eps and k >= times:
            return k
    return None


@functools.lru_cache(maxsize=None)
def problem(n, P):
    """(csr, gamma, X0) of the circulant graph at n agents x P parameters: built once, shared,
    never modified."""
    csr = circulant_csr(n)
    X0 = np.random.default_rng(n * 7 + P).standard_normal((n, P), dtype=np.float32)
    X0.setflags(write=False)
    return csr, spectral_radius(csr), X0


def margin_eps(devs, below):
    """(k*, eps) for a device run of the loop that must stop at the oracle's round: k* the first
    round whose deviation is a new running minimum below ``below`` such that eps, the geometric
    mean of it and the smallest earlier deviation, has every earlier deviation above 1.01 eps and
    d_k* below 0.99 eps -- a device deviation within 1e-5 relative then cannot move the count."""
    for k in range(1, len(devs)):
        lo = min(devs[:k])
        if devs[k] < lo and devs[k] < below:
            eps = float(np.sqrt(devs[k] * lo))
            if lo > 1.01 * eps and devs[k] < 0.99 * eps:
                return k + 1, eps
    raise AssertionError("no round with a 1 % gap on both sides")
