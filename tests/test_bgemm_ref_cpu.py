"""The dl_bgemm oracle by itself (oracle/mix_ref.c ref_bgemm, no GPU): the fp32 fma chain stays
within its derived forward-error bound of numpy float64 on every case the GPU tests use, the
four ta/tb storage variants of one logical product give identical bits, and the epilogues are
the single-rounding expressions that include/dlamd.h describes."""
import numpy as np
import pytest

import bgemm_cases as bc
from bgemm_cases import EPI, U

ALL_CASES = bc.LINEAR_CASES + bc.DTANH_CASES + bc.ACT_CASES


def test_case_lists_cover_what_they_claim():
    """The case lists are designed, not a product: every boundary size appears at least once."""
    gemm = ALL_CASES + [bc.Case(c.M, c.N, c.K, c.batch, c.ta, c.tb, "bias_xent")
                        for c in bc.XENT_CASES]
    sizes = {1, 15, 17, 63, 64, 65, 150, 161}
    assert sizes <= {c.M for c in bc.LINEAR_CASES} and sizes <= {c.N for c in bc.LINEAR_CASES}
    assert {1, 3, 31, 32, 33, 64, 95} <= {c.K for c in bc.LINEAR_CASES}
    assert {1, 3, 9} <= {c.batch for c in bc.LINEAR_CASES}
    assert {(c.ta, c.tb) for c in bc.LINEAR_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c.epi for c in gemm} == set(EPI)
    # 64 x 64 tiles: fewer than 8 workgroups, more than 8 with a remainder; exactly 8 on 16 x 64
    grids = {bc.grid_size(c) for c in bc.LINEAR_CASES if c.shape is None}
    assert 1 in grids and {9, 12, 81} <= grids
    assert any(c.shape == 5 and bc.grid_size(c, 16, 64) == 8 for c in bc.LINEAR_CASES)
    for ta in (0, 1):          # rowsum with both storages, several tiles in y and in x
        assert any(c.rowsum and c.ta == ta and c.M > 64 for c in bc.LINEAR_CASES)
        assert any(c.rowsum and c.ta == ta and c.N > 64 for c in bc.LINEAR_CASES)
    assert {c.M for c in bc.XENT_CASES} == {1, 5, 63, 64}
    assert {c.N for c in bc.XENT_CASES} == {1, 2, 7, 63, 64}
    assert {c.classes for c in bc.XENT_GRAD_CASES} == {1, 2, 10, 63, 64}
    assert {c.rows for c in bc.XENT_GRAD_CASES} == {1, 3, 4, 5, 65, 130}
    assert {c.batch for c in bc.XENT_GRAD_CASES} == {1, 3}
    assert max(c.M * c.N * c.K * c.batch for c in gemm) <= 25_000_000


@pytest.mark.parametrize("c", ALL_CASES, ids=bc.case_id)
def test_fma_chain_within_its_error_bound_and_storage_independent(c):
    """|c_hat - c| <= (K + 2) 2^-24 (sum_k |a_k||b_k| + |bias_n|): gamma_K of a length-K fma
    chain with u = 2^-24, one more rounding for the bias add (derived, not measured).  The
    operands stored as ta/tb say -- four layouts of the same numbers -- give the same bits."""
    p = bc.linear_problem(c, seed=1)
    # the chain and the bias add, whatever the case's own epilogue does afterwards
    epi = "none" if p.bias_v is None else "bias"
    q = bc.Problem(p.M, p.N, p.K, p.batch, p.ta, p.tb, epi, p.opA, p.opB, p.bias_v)
    got = q.oracle()[0]
    exact, mag = bc.product_f64(q)
    if p.bias_v is not None:
        exact = exact + p.bias_v[:, None, :].astype(np.float64)
        mag = mag + np.abs(p.bias_v[:, None, :]).astype(np.float64)
    assert np.all(np.abs(got.astype(np.float64) - exact) <= (c.K + 2) * U * mag)
    for ta in (0, 1):
        for tb in (0, 1):
            other = bc.restored(q, ta, tb).oracle()[0]
            assert np.array_equal(other.view(np.uint32), got.view(np.uint32)), (ta, tb)


@pytest.mark.parametrize("c", ALL_CASES, ids=bc.case_id)
def test_epilogues_are_single_roundings_of_the_chain(c):
    """Each epilogue restated in numpy fp32 from the NONE result (numpy rounds every operation
    once); BIAS_TANH / BIAS_ELU / BIAS_XENT return the pre-activation; bias NULL adds nothing;
    rowsum is the k-ordered fp32 sum, within (K - 1) u sum|a| of float64."""
    p = bc.linear_problem(c, seed=2)
    got, got2, rs = p.oracle()
    acc = bc.Problem(p.M, p.N, p.K, p.batch, p.ta, p.tb, "none", p.opA, p.opB).oracle()[0]
    one, zero = np.float32(1), np.float32(0)
    z = acc + p.bias_v[:, None, :] if p.bias_v is not None else acc
    h = p.H_v
    want = {"none": lambda: acc, "bias": lambda: z, "bias_tanh": lambda: z,
            "bias_elu": lambda: z, "bias_relu": lambda: np.where(z > 0, z, zero),
            "drelu": lambda: acc * np.where(h > 0, one, zero),
            "delu": lambda: acc * np.where(h > 0, one, h + one),
            "dtanh": lambda: acc * (one - h * h)}[c.epi]()
    assert want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if c.epi == "dtanh":
        fused = (1.0 - h.astype(np.float64) ** 2).astype(np.float32)   # exact in fp64: one rounding
        assert np.array_equal(got2.view(np.uint32), (acc * fused).view(np.uint32))
        assert not np.array_equal(got2.view(np.uint32), got.view(np.uint32))
    if c.rowsum:
        s = np.zeros((c.batch, c.M), np.float32)
        for k in range(c.K):
            s = s + p.opA[:, :, k]
        assert np.array_equal(rs.view(np.uint32), s.view(np.uint32))
        a64 = p.opA.astype(np.float64)
        assert np.all(np.abs(rs - a64.sum(axis=2)) <= c.K * U * np.abs(a64).sum(axis=2))


def test_xent_pre_activation_is_the_biased_chain():
    c = bc.XENT_CASES[3]
    p = bc.xent_problem(c, seed=3)
    z = p.oracle()[0]
    q = bc.Problem(p.M, p.N, p.K, p.batch, p.ta, p.tb, "bias", p.opA, p.opB, p.bias_v)
    assert np.array_equal(z.view(np.uint32), q.oracle()[0].view(np.uint32))


def test_xent_inputs_keep_the_loss_well_conditioned():
    """The loss is held to a relative tolerance on the GPU; that presupposes a mean loss far above
    the fp32 resolution of logsumexp(z) - z[label] (about 2^-23 max|z|).  The inputs are drawn so
    (order-one logits, the spread's largest offset off the planted label lanes); a single class
    gives exactly 0."""
    for i, c in enumerate(bc.XENT_CASES):
        p = bc.xent_problem(c, seed=100 + i)
        z = p.oracle()[0]
        _, loss = bc.xent_reference(z, p.labels[:, :c.M])
        assert np.all(loss == 0) if c.N == 1 else np.all(loss > 0.25), (c, loss)
        if c.spread:
            assert np.all(z.max(axis=2) - z.min(axis=2) > 2 * c.spread - 16)
    for i, c in enumerate(bc.XENT_GRAD_CASES):
        Z, lab = bc.xent_grad_logits(c, seed=200 + i)
        _, loss = bc.xent_reference(Z, lab)
        assert np.all(loss == 0) if c.classes == 1 else np.all(loss > 0.25), (c, loss)
