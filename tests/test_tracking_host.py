"""The algorithm dl_track_round must reproduce, pinned on the CPU with the oracle alone
(track_oracle.track_step): on quadratic losses f_a(x) = 1/2 ||x - c_a||^2 with different c_a per
agent, constant-step gradient tracking reaches the optimum mean(c) where the plain round
W (X - lr G) stalls at its bias, and the tracker's network mean equals the gradients' at every
step.  The oracle gives 2.2e-6 (circulant, 16 agents) and 8.3e-7 (random 4-regular, 64 agents)
against 1.2 and 1.3 for the plain round after 300 rounds, and a mean gap of at most 2.2e-7."""
import numpy as np
import pytest

import track_oracle as O
from cheb_oracle import circulant_csr

P, LR, ROUNDS = 16, 0.1, 300
GRAPHS = {"circulant16": lambda: circulant_csr(16),
          "regular64": lambda: O.uniform_regular_csr(64, 4, seed=0)}


@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_tracking_reaches_the_optimum_and_the_plain_round_does_not(graph):
    csr = GRAPHS[graph]()
    assert csr.doubly_stochastic and csr.uniform_row_nnz == 5
    assert np.all(csr.w.astype(np.float32) == np.float32(0.2))
    n = csr.n_rows
    c = O.quadratic_targets(n, P)
    worst = [0.0]

    def mean_is_tracked(X, D, G):
        gap = np.max(np.abs(D.astype(np.float64).mean(axis=0) - G.astype(np.float64).mean(axis=0)))
        worst[0] = max(worst[0], gap / max(1.0, float(np.max(np.abs(G)))))
    X, _ = O.tracked_run(csr, c, LR, ROUNDS, on_round=mean_is_tracked)
    tracked, plain = O.distance(X, c), O.distance(O.plain_run(csr, c, LR, ROUNDS), c)
    print(f"{graph}: tracked {tracked:.3e}, plain {plain:.3e}, mean gap {worst[0]:.3e}")
    assert tracked < 1e-4
    assert plain > 0.1
    # max_j |mean_a D - mean_a G| <= 1e-5 max(1, max |G|) at every step
    assert worst[0] <= 1e-5


def test_first_round_is_the_mixed_gradient():
    """From D = 0 and Gold = 0 the first tracker is W g exactly: no `first` flag."""
    from oracle import cref
    csr = circulant_csr(16)
    c = O.quadratic_targets(16, P)
    X0 = np.zeros_like(c)
    G = O.quadratic_grad(X0, c)
    _, D = O.track_step(csr, X0, np.zeros_like(c), G, np.zeros_like(c), LR)
    assert np.array_equal(D.view(np.uint32),
                          cref.mix_round(G, csr.rowptr, csr.col, csr.w).view(np.uint32))
