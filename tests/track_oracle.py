"""numpy restatement of the gradient-tracking round (dl_track_round, include/dlamd.h), shared by
test_tracking_host.py and test_track_round_gpu.py: the four lines of the definition with fp32
element-wise numpy operations and the oracle's fold (cref.mix_round, bit for bit
Mixer._mix_params_once; its fused step for the parameters), and the quadratic problem whose optimum
the tracked iterates reach and the plain round's do not."""
import functools

import numpy as np

from oracle import cref


def track_step(csr, X, D, G, Gold, lr):
    """(X', D') of one round: t = fl(fl(d + g) - q), d' = W t, x' = W fl(x - fl(lr d'))."""
    f32 = lambda a: np.asarray(a, np.float32)
    T = (f32(D) + f32(G)) - f32(Gold)
    assert T.dtype == np.float32
    Dn = cref.mix_round(T, csr.rowptr, csr.col, csr.w)
    Xn = cref.mix_round(f32(X), csr.rowptr, csr.col, csr.w, G=Dn, lr=lr)
    return Xn, Dn


def plain_step(csr, X, G, lr):
    """The plain round X' = W (X - lr G) (decentralized gradient descent)."""
    return cref.mix_round(np.asarray(X, np.float32), csr.rowptr, csr.col, csr.w,
                          G=np.asarray(G, np.float32), lr=lr)


@functools.lru_cache(maxsize=None)
def quadratic_targets(n, P):
    """c of f_a(x) = 1/2 ||x - c_a||^2: built once, shared, never modified.  The optimum of the
    summed loss is mean_a c_a."""
    c = (np.random.default_rng(n + P).standard_normal((n, P)) * 3).astype(np.float32)
    c.setflags(write=False)
    return c


def quadratic_grad(X, c):
    """The agents' gradients fl(x_a - c_a)."""
    return np.asarray(X, np.float32) - c


def tracked_run(csr, c, lr, rounds, on_round=None):
    """``rounds`` tracked rounds on the quadratic problem from X = 0, D = 0, Gold = 0.  Returns
    (X, D); on_round(X, D, G) sees every round's state and the gradient it used."""
    X = np.zeros_like(c)
    D = np.zeros_like(c)
    Gold = np.zeros_like(c)
    for _ in range(rounds):
        G = quadratic_grad(X, c)
        X, D = track_step(csr, X, D, G, Gold, lr)
        if on_round is not None:
            on_round(X, D, G)
        Gold = G
    return X, D


def plain_run(csr, c, lr, rounds):
    X = np.zeros_like(c)
    for _ in range(rounds):
        X = plain_step(csr, X, quadratic_grad(X, c), lr)
    return X


def distance(X, c):
    """max_a,j |x_a - mean(c)| against the fp64 optimum."""
    return float(np.max(np.abs(X.astype(np.float64) - c.astype(np.float64).mean(axis=0))))


def uniform_regular_csr(n, deg=4, seed=0):
    """A random `deg`-regular undirected graph on n agents with the uniform weight 1 / (deg + 1) on
    every edge and the diagonal: symmetric, so doubly stochastic.  Built as the union of deg / 2
    random Hamiltonian cycles, redrawn until no edge repeats."""
    from distributed_learning_amd.graph import Csr
    assert deg % 2 == 0 and n > deg
    rng = np.random.default_rng(seed)
    while True:
        nbrs = [set() for _ in range(n)]
        ok = True
        for _ in range(deg // 2):
            p = rng.permutation(n)
            for i in range(n):
                a, b = int(p[i]), int(p[(i + 1) % n])
                if b in nbrs[a]:
                    ok = False
                nbrs[a].add(b)
                nbrs[b].add(a)
        if ok and all(len(s) == deg for s in nbrs):
            break
    cl = np.concatenate([[a] + sorted(nbrs[a]) for a in range(n)])
    csr = Csr(np.arange(0, (deg + 1) * n + 1, deg + 1), cl, np.full(cl.size, 1.0 / (deg + 1)))
    assert csr.doubly_stochastic and csr.uniform_row_nnz == deg + 1
    return csr
