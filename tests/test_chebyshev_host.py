"""Host-side checks of the Chebyshev-accelerated gossip (no GPU): the relaxation factors, the
symmetry test of a Csr, and that a numpy restatement of GossipEngine.mix_chebyshev (the oracle's
fold, the rounding rule of include/dlamd.h) reaches eps in at most a quarter of the plain loop's
rounds on the tests' circulant graph."""
import math

import numpy as np
import pytest

import cheb_oracle as O


@pytest.mark.parametrize("gamma", [0.5, 0.964119, 0.990388, 0.999])
def test_chebyshev_omegas(gamma):
    from distributed_learning_amd.utils.fast_averaging import chebyshev_omegas
    om = chebyshev_omegas(gamma, 200)
    assert len(om) == 200 and all(isinstance(w, float) for w in om)
    assert om[0] == 1.0 and om[1] == 2.0 / (2.0 - gamma * gamma)
    for j in range(2, 200):
        assert om[j] == 4.0 / (4.0 - gamma * gamma * om[j - 1])
    # monotone towards the fixed point 1 + rho^2 of w = 4 / (4 - gamma^2 w)
    rho = gamma / (1.0 + math.sqrt(1.0 - gamma * gamma))
    limit = 1.0 + rho * rho
    assert limit == pytest.approx(4.0 / (4.0 - gamma * gamma * limit), rel=1e-14)
    # from w_2 on (w_1 = 1 is the plain round)
    assert om[1] > limit > om[0]
    assert all(a >= b for a, b in zip(om[1:], om[2:]))
    assert all(w >= limit * (1 - 1e-15) for w in om[1:])
    gaps = [w - limit for w in om[1:40]]
    assert all(g2 < g1 for g1, g2 in zip(gaps, gaps[1:]) if g1 > 1e-13)
    assert om[-1] == pytest.approx(limit, rel=1e-6 if gamma > 0.99 else 1e-12)
    # a prefix is a prefix
    assert chebyshev_omegas(gamma, 5) == om[:5] and chebyshev_omegas(gamma, 0) == []
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            chebyshev_omegas(bad, 3)


def test_csr_symmetric():
    from distributed_learning_amd.graph import Csr
    assert O.circulant_csr(33).symmetric and O.circulant_csr(64).symmetric
    # symmetric with rows of different lengths and entry orders
    sym = Csr([0, 2, 5, 7], [0, 1, 2, 0, 1, 2, 1], [0.5, 0.5, 0.25, 0.5, 0.25, 0.75, 0.25])
    assert sym.symmetric and sym.doubly_stochastic
    # row-stochastic only: the pattern is symmetric, the weights are not
    rs = Csr([0, 2, 5, 7], [0, 1, 2, 0, 1, 2, 1], [0.5, 0.5, 0.25, 0.25, 0.5, 0.75, 0.25])
    assert not rs.symmetric and not rs.doubly_stochastic
    assert np.allclose(rs.dense().sum(axis=1), 1.0)
    # an entry without its mirror
    assert not Csr([0, 2, 3], [0, 1, 1], [0.5, 0.5, 1.0]).symmetric
    # halo columns: not a square W
    assert not Csr([0, 1], [1], [1.0], n_src=2).symmetric


@pytest.mark.parametrize("n,P,gamma", [(64, 256, 0.990388), (33, 129, 0.964119)])
def test_restated_loop_needs_a_quarter_of_the_rounds(n, P, gamma):
    csr, g, X0 = O.problem(n, P)
    assert g == pytest.approx(gamma, abs=1e-6)
    eps = 1e-2
    rho = g / (1.0 + math.sqrt(1.0 - g * g))
    d0 = O.max_deviation(X0)
    # rounds the contraction factors predict (the iterate's deviation <= 2 rho^k d0 for the
    # semi-iteration, gamma^k d0 for the plain loop), with room for fp32 and the transient
    k_cheb = math.ceil(math.log(2.0 * d0 / eps) / -math.log(rho)) + 2
    k_plain = math.ceil(math.log(d0 / eps) / -math.log(g)) + 2
    cheb = O.rounds_until([d for _, d in O.cheb_rounds(csr, X0, g, k_cheb)], eps)
    plain = O.rounds_until([d for _, d in O.plain_rounds(csr, X0, k_plain)], eps)
    print(f"n={n} P={P} gamma={g:.6f} eps={eps}: plain {plain} rounds, Chebyshev {cheb}")
    assert cheb is not None and plain is not None
    assert 4 * cheb <= plain
    # the mean is kept (a + b = 1) to fp32 rounding
    Xc = O.cheb_rounds(csr, X0, g, cheb)[-1][0]
    np.testing.assert_allclose(Xc.astype(np.float64).mean(axis=0),
                               X0.astype(np.float64).mean(axis=0), atol=1e-5)


def test_engine_refuses_bad_gamma_and_asymmetric_w():
    """mix_chebyshev's argument checks come before any device work (checked on the class)."""
    from distributed_learning_amd import engine

    class Fake:
        class W:
            csr = None
    f = Fake()
    f.W.csr = O.circulant_csr(8)
    for bad in (0.0, 1.0, -0.5, 2.0):
        with pytest.raises(ValueError, match="gamma"):
            engine.GossipEngine.mix_chebyshev(f, bad)
    from distributed_learning_amd.graph import Csr
    f.W.csr = Csr([0, 2, 5, 7], [0, 1, 2, 0, 1, 2, 1], [0.5, 0.5, 0.25, 0.25, 0.5, 0.75, 0.25])
    with pytest.raises(ValueError, match="symmetric"):
        engine.GossipEngine.mix_chebyshev(f, 0.9)
