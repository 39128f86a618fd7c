"""The numpy oracle of the c1 kernels (tests/jacobi_oracle.py) and the inputs of their GPU tests
(tests/jacobi_cases.py), checked on the CPU:

* the CSR oracle equals oracle/mixer_ref.jacobi_round (pinned to the reference's runs) bit for
  bit, values and iteration count, fp64 and fp32, with and without weights;
* the numpy facts the kernels restate: NEP 50 dtypes of the fp32 oracle, the +0.0 start of
  np.sum, the pairwise reduction of a stack of scalars;
* no GPU case sits on a knife edge: every convergence test of every iteration is at least 1e-6
  relative away from its conv_eps, and the consensus-GD oracle's own summation error (against
  np.longdouble dot products) is a tenth of the bound the kernel is held to."""
import numpy as np
import pytest

import jacobi_cases as C
import jacobi_oracle as O
from oracle import mixer_ref as M


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", list(O.GRAPHS))
def test_csr_oracle_equals_mixer_ref(name, dt, weights):
    """fp64: mixer_ref.jacobi_round as the golden tests call it (eps a numpy float64 scalar, as
    in the reference).  fp32: the same function with eps passed as a Python float through
    ``edge_weight`` -- a numpy float64 eps is strong and would promote the float32 values to
    float64, while the fp32 kernel keeps every operation in float32, which under NEP 50 is the
    same expression with weak (Python) scalars."""
    edges, dtype = O.GRAPHS[name], C.DTYPES[dt]
    toks, rowptr, col = O.csr_from_edges(edges)
    n = len(toks)
    V = np.random.default_rng(n).standard_normal((n, 5)).astype(dtype)
    wts = list(range(1, n + 1)) if weights else [1] * n
    want, k_ref = M.jacobi_round(edges, {t: V[i] for i, t in enumerate(toks)},
                                 {t: wts[i] for i, t in enumerate(toks)}, 5e-2, max_iter=64,
                                 edge_weight=None if dt == "f64" else O.max_degree_eps(rowptr))
    assert O.max_degree_eps(rowptr) == float(M.perron_eps(edges, toks))
    got, k = O.jacobi_round(V, rowptr, col, O.max_degree_eps(rowptr), 5e-2,
                            weight=wts if weights else None, mean_w=sum(wts) / n, max_iter=64)
    assert 1 < k == k_ref < 64
    assert got.dtype == dtype and all(want[t].dtype == dtype for t in toks)
    assert O.same_bits(got, np.stack([want[t] for t in toks]))


def test_fp32_oracle_stays_fp32():
    """NEP 50: Python-float eps, conv_eps, weight and mean_w next to float32 arrays are cast to
    float32 -- the kernels' (DT) casts -- in the products, the division and the comparison."""
    v = np.arange(1, 4, dtype=np.float32)
    assert O.prescale(v, 3.0, 4.5).dtype == np.float32
    assert np.array_equal(O.prescale(v, 3.0, 4.5), v * np.float32(3.0) / np.float32(4.5))
    assert (v * (1 - 0.475 * 2) + 0.475 * v).dtype == np.float32
    assert (0.1 * v)[0] == np.float32(0.1) and float((0.1 * v)[0]) != 0.1
    # the comparison rounds conv_eps to float32 too: 1 <= fl32(0.99999999999) == 1
    assert np.all(np.ones(2, np.float32) <= 0.99999999999)
    assert not np.any(np.ones(2, np.float64) <= 0.99999999999)
    Y, _ = O.jacobi_step(np.ones((8, 3), np.float32), *O.ring_csr(8), 0.475, conv_eps=1e-3)
    assert Y.dtype == np.float32
    # a numpy float64 scalar is strong: the reason every scalar passes through float()
    assert (v * np.float64(3.0)).dtype == np.float64


def test_np_sum_starts_at_plus_zero():
    """np.sum(list, axis=0) folds from +0.0: neighbours that all hold -0.0 sum to +0.0, as
    vectors and as a stack of scalars (sequential below 8 terms, pairwise from 8)."""
    z = np.array([-0.0, -0.0])
    s = np.sum([z, z, z], axis=0)
    assert np.array_equal(s, [0.0, 0.0]) and not np.signbit(s).any()
    for d in (3, 9):
        for dtype in (np.float64, np.float32):
            assert not np.signbit(np.sum([dtype(-0.0)] * d, axis=0))
    # and so does the oracle's step: an all -0.0 column comes out +0.0
    Y = np.full((8, 2), -0.0)
    new, fail = O.jacobi_step(Y, *O.ring_csr(8), 0.475, conv_eps=1e-3)
    assert not fail and not np.signbit(new).any()


@pytest.mark.parametrize("f32", [0, 1])
def test_pairwise_sum_differs_from_left_fold(f32):
    """The n_params == 1 draws can tell numpy's pairwise reduction from a left fold for some
    d >= 8, equal it below 8, and a (d, 1) stack reduces like a (d,) stack."""
    dtype = np.float32 if f32 else np.float64
    differ = []
    for d in C.ASYNC_D[1:]:
        v = [dtype(x) for x in C.async_scalars(d, f32)[1:]]
        pair = np.sum(v, axis=0)
        assert pair.dtype == dtype
        assert pair == np.sum([np.array([x]) for x in v], axis=0)[0]
        if d < 8:
            assert pair == O.left_fold(v)
        elif pair != O.left_fold(v):
            differ.append(d)
    assert differ, "no d >= 8 separates pairwise from sequential summation"


def test_planner_widths():
    """The boundary cases stand where the planner's formula 2 R P sz + 16 <= kLdsBytes puts
    them: the last single-launch width, and one past it a tile wider than the matrix."""
    assert C.single_limit(np.float64, 64) == 159 and C.single_limit(np.float32, 64) == 319
    assert C.perron_tile_cols(np.float64, 64, 159) == 159
    assert C.perron_tile_cols(np.float64, 64, 160) == 319
    assert C.perron_tile_cols(np.float32, 64, 319) == 319
    assert C.perron_tile_cols(np.float32, 64, 320) == 639
    assert C.perron_tile_cols(np.float64, 64, 700) == 319 and 700 == 2 * 319 + 62
    assert C.perron_tile_cols(np.float32, 64, 1300) == 639 and 1300 == 2 * 639 + 22
    assert C.ROW_LIMIT == 20478
    assert C.perron_tile_cols(np.float64, C.ROW_LIMIT, 3) == 1
    assert C.perron_tile_cols(np.float64, C.ROW_LIMIT + 1, 3) == 0
    assert C.perron_tile_cols(np.float64, 8, 33) == 33 == C.perron_tile_cols(np.float32, 8, 33)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", list(C.PERRON_CASES))
def test_perron_cases_have_margin(name, dt):
    spec, c = C.PERRON_CASES[name], C.perron_case(name, dt)
    Y, k = c["want"]
    assert Y.dtype == c["dtype"] and len(c["trace"]) == k <= 64 and c["max_iter"] <= 64
    top = [float(np.max(g)) for g in c["trace"]]
    if "cut" in spec:
        # conv_eps = 0: every iteration fails by far, the loop ends at max_iter
        assert k == spec["cut"] and min(top) > 1e-3
    elif "special" in spec:
        # a NaN (at once, or from inf - inf) fails every iteration's test
        assert k == c["max_iter"] == spec["max_iter"] and np.isnan(Y).any()
    else:
        assert O.margin(c["trace"], c["conv_eps"], c["conv_rows"]) >= C.MARGIN
        assert k < c["max_iter"]
        if "k" in spec:
            assert k == spec["k"]
        else:
            # the one strict agent decides: without it the round stops at k_loose
            row, k_loose, _ = spec["strict"]
            assert k > k_loose
            assert all(np.all(np.delete(g, row) <= np.delete(c["conv_rows"], row))
                       for g in c["trace"][k_loose - 1:])
            assert c["trace"][k - 2][row] > c["conv_rows"][row]
    if spec.get("special") == "negzero":
        # the oracle's answer where a whole neighbourhood holds -0.0 is +0.0
        assert np.signbit(c["Y0"][:, 1]).all() and not np.signbit(Y[:, 1]).any()
        if k == 1:
            assert Y[5, c["P"] - 2] == 0 and not np.signbit(Y[5, c["P"] - 2])


def test_row_limit_case():
    c = C.row_limit_case()
    assert c["want"][1] == 2 and c["Y0"].shape == (20478, 3)


@pytest.mark.parametrize("name", list(C.GD_CASES))
def test_consensus_gd_cases(name):
    """Jacobi counts are off every knife edge, and the fp64 oracle does not consume the kernel's
    bound (rtol 1e-9, atol 1e-12): with the gradient's dot products in np.longdouble it moves by
    less than a tenth of it, and no count changes."""
    c = C.gd_case(name)
    W, ks, trace = C.gd_want(name)
    Wl, ksl, _ = C.gd_want(name, True)
    assert ks == ksl and len(ks) == len(c["steps"])
    np.testing.assert_allclose(W, Wl, rtol=1e-10, atol=1e-13)
    assert np.all(c["W0"] != 0) and np.isfinite(W).all() and max(ks) <= c["max_iter"] <= 64
    if c["conv_eps"] == 0.0:
        assert ks == [c["max_iter"]] * len(ks)
        assert min(float(np.max(g)) for g in trace) > 1e-3
    else:
        assert max(ks) < c["max_iter"]
        assert O.margin(trace, c["conv_eps"]) >= C.MARGIN
    rows = int(c["sp"][-1])
    in_lds = C.gd_lds_bytes(c["R"], c["F"], rows, True) <= C.K_LDS_BYTES
    assert in_lds == (name != "c_global_f16")
    assert C.gd_lds_bytes(c["R"], c["F"], rows, False) <= C.K_LDS_BYTES
    if name == "c_global_f16":
        assert rows * (c["F"] + 1) * 8 > C.K_LDS_BYTES
    sizes = np.diff(c["sp"])
    if name in ("crosscheck", "a_ring12_f16"):
        assert c["R"] > 8 and {1, 2, 63, 64, 65} <= set(sizes.tolist())
    if name == "d_isolated":
        assert (np.diff(c["rowptr"]) == 0).sum() == 1
