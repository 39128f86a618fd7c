"""dl_bgemm and dl_xent_grad called directly (not through BatchedANN) against the fma-chain
oracle of oracle/mix_ref.c (ref_bgemm), on the case lists of tests/bgemm_cases.py.

include/dlamd.h promises "fp32 MFMA (16x16x4), exact fp32 products" and csrc/bgemm.hip "a
k-ordered f32 fma chain": the epilogues that are rounded fp32 expressions of that chain (NONE,
BIAS, BIAS_RELU, DRELU, DELU, DTANH) and rowsum are compared BIT FOR BIT, for the four ta/tb
storages and the six tile shapes (DLAMD_BGEMM_SHAPE).  For BIAS_TANH, BIAS_ELU and BIAS_XENT the
oracle gives the bit-defined pre-activation z; the activation / softmax cross-entropy is then
taken from that z in float64, so only the device's tanhf, expm1f, expf and logf are under a
tolerance.  Every operand sits in a NaN-padded buffer and every output buffer must come back
bit-unchanged outside its logical elements.
"""
import ctypes

import numpy as np
import pytest
import torch

import bgemm_cases as bc

pytestmark = pytest.mark.gpu

# BIAS_TANH / BIAS_ELU against float64 tanh / expm1 of the oracle's z, in ulps of the fp32
# result.  Cap = 2 x the largest distance observed over ACT_CASES on an MI355X with the kernels
# of commit 8251639 (unchanged by the commit that adds this file): 1.276 ulp (tanhf, case
# 17x161x33b1-tn; expm1f at most 0.825).  Anything above 16 ulp would mean a wrong activation,
# not an imprecise one (the GEMM part is pinned bit-exactly), and must not be recorded here.
ACT_ULP_OBSERVED = 1.276
ACT_ULP_CAP = 2 * ACT_ULP_OBSERVED
# BIAS_XENT / dl_xent_grad: |dZ * rows - (softmax - onehot)| against float64 from the exact
# logits.  Cap = 2 x the largest error observed over XENT_CASES and XENT_GRAD_CASES (same
# machine and commit): 1.195e-7 (M 64, N 63, logits spread over +-80); a value above 1e-5 must
# not be recorded.  The loss was within 1.1e-7 relative everywhere.
DZ_ABS_OBSERVED = 1.195e-7
DZ_ABS_CAP = 2 * DZ_ABS_OBSERVED
LOSS_REL = 1e-5      # the project's figure (test_gradients_match_autograd)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(got, want, what):
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements differ, max abs "
                           f"difference {np.nanmax(np.abs(got[bad] - want[bad])):.3e}")


def _dev(buf, cuda):
    return torch.from_numpy(buf).to(cuda) if buf is not None else None


def run_bgemm(p, cuda, with_loss=True):
    """One dl_bgemm launch of Problem p into fresh sentinel buffers -> host copies of the
    whole C, rowsum and loss buffers (padding included)."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    A, B, C = _dev(p.A.buf, cuda), _dev(p.B.buf, cuda), _dev(p.C.buf, cuda)
    bias = _dev(p.bias.buf, cuda) if p.bias else None
    H = _dev(p.H.buf, cuda) if p.H else None
    rs = _dev(p.rowsum.buf, cuda) if p.rowsum else None
    labels = _dev(p.labels, cuda)
    loss = None
    if p.want_loss and with_loss:
        loss = torch.from_numpy(np.full(p.batch + 4, bc.SENTINEL, np.uint32).view(np.float32)
                                ).to(cuda)
    args = _lib.DlBgemmArgs(
        batch=p.batch, M=p.M, N=p.N, K=p.K, A=_lib.ptr(A), lda=p.A.ld, sA=p.A.stride, ta=p.ta,
        B=_lib.ptr(B), ldb=p.B.ld, sB=p.B.stride, tb=p.tb, C=_lib.ptr(C), ldc=p.C.ld,
        sC=p.C.stride, epi=p.epi, bias=_lib.ptr(bias), s_bias=p.bias.stride if p.bias else 0,
        H=_lib.ptr(H), ldh=p.H.ld if p.H else 0, sH=p.H.stride if p.H else 0,
        rowsum=_lib.ptr(rs), s_rowsum=p.rowsum.stride if p.rowsum else 0,
        labels=_lib.ptr(labels), s_labels=p.labels.shape[1] if p.labels is not None else 0,
        loss=_lib.ptr(loss))
    _lib.check(lib.dl_bgemm(ctypes.byref(args), _lib.stream_handle(cuda)), "dl_bgemm")
    torch.cuda.synchronize()
    for t, src in ((A, p.A.buf), (B, p.B.buf)):       # inputs are only read
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(src))
    return (C.cpu().numpy(), rs.cpu().numpy() if rs is not None else None,
            loss.cpu().numpy() if loss is not None else None)


def run_twice(p, cuda):
    """Two launches into fresh buffers: identical bits (determinism), padding untouched."""
    c1, r1, l1 = run_bgemm(p, cuda)
    c2, r2, l2 = run_bgemm(p, cuda)
    assert np.array_equal(_bits(c1), _bits(c2)), "C differs between two launches"
    assert p.C.padding_intact(c1), "C written outside its M x N logical elements"
    if r1 is not None:
        assert np.array_equal(_bits(r1), _bits(r2)), "rowsum differs between two launches"
        assert p.rowsum.padding_intact(r1), "rowsum written outside its M elements"
    if l1 is not None:
        assert np.array_equal(_bits(l1), _bits(l2)), "loss differs between two launches"
        assert np.all(_bits(l1)[p.batch:] == bc.SENTINEL), "loss written past [batch]"
    return (p.C.logical(c1).copy(), p.rowsum.logical(r1)[:, 0, :].copy() if r1 is not None
            else None, l1[:p.batch].copy() if l1 is not None else None)


def check_linear(p, cuda, what):
    want, _, want_rs = p.oracle()
    got, got_rs, _ = run_twice(p, cuda)
    _same_bits(got, want, f"{what} C")
    if want_rs is not None:
        _same_bits(got_rs, want_rs, f"{what} rowsum")


def _set_shape(monkeypatch, shape):
    if shape is None:
        monkeypatch.delenv("DLAMD_BGEMM_SHAPE", raising=False)
    else:
        monkeypatch.setenv("DLAMD_BGEMM_SHAPE", f"{shape},{shape}")


@pytest.mark.parametrize("c", bc.LINEAR_CASES, ids=bc.case_id)
def test_linear_epilogues_and_rowsum_equal_the_fma_chain(cuda, monkeypatch, c):
    """NONE, BIAS (also with bias = NULL), BIAS_RELU, DRELU, DELU and rowsum: the bits of the
    k-ordered fma chain, twice, with nothing written outside the logical elements."""
    _set_shape(monkeypatch, c.shape)
    check_linear(bc.linear_problem(c, seed=10), cuda, bc.case_id(c))


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("shape", range(6))
def test_every_tile_shape_and_storage_gives_the_same_bits(cuda, monkeypatch, shape, ta, tb):
    """Tile shapes 0-5 x the four ta/tb instantiations, at a size on each side of M = 64 (the
    `small` and the `large` selector of bgemm_shape): the fma chain does not depend on either."""
    _set_shape(monkeypatch, shape)
    for i, (M, N, K, batch, epi) in enumerate(bc.SHAPE_SIZES):
        c = bc.Case(M, N, K, batch, ta, tb, epi, rowsum=True)
        check_linear(bc.linear_problem(c, seed=20 + i), cuda, bc.case_id(c))


@pytest.mark.parametrize("c", bc.DTANH_CASES, ids=bc.case_id)
def test_dtanh_is_one_of_the_two_roundings(cuda, monkeypatch, c):
    """acc * (1 - h h): each element is acc * fl(1 - fl(h h)) or acc * fma(-h, h, 1) (the device
    compiler may contract the expression), nothing else."""
    _set_shape(monkeypatch, None)
    p = bc.linear_problem(c, seed=30)
    plain, fused, _ = p.oracle()
    got, _, _ = run_twice(p, cuda)
    ok = (_bits(got) == _bits(plain)) | (_bits(got) == _bits(fused))
    assert ok.all(), f"{int((~ok).sum())} of {ok.size} elements match neither candidate"


@pytest.mark.parametrize("c", bc.ACT_CASES, ids=bc.case_id)
def test_forward_activations_of_the_exact_pre_activation(cuda, monkeypatch, c):
    """BIAS_TANH / BIAS_ELU: tanhf / expm1f of the bit-defined z against float64, in ulps."""
    _set_shape(monkeypatch, None)
    p = bc.linear_problem(c, seed=40)
    z = p.oracle()[0].astype(np.float64)
    ref = np.tanh(z) if c.epi == "bias_tanh" else np.where(z > 0, z, np.expm1(z))
    if not c.bias_null and c.M * c.N * c.batch > 100:
        # the inputs do reach z around 0, z large negative (ELU -> -1) and |z| large (tanh -> +-1)
        assert (np.abs(z) < 2.0 ** -6).any() and (z < -20).any() and (z > 20).any()
    got, _, _ = run_twice(p, cuda)
    assert np.isfinite(got).all()
    d = bc.ulp_distance(got, ref)
    print(f"\n[measure] {bc.case_id(c)} max ulp {d.max():.3f}")
    assert d.max() <= ACT_ULP_CAP


def _check_xent(dz, loss, z, labels, rows, what):
    """dZ [batch][rows][classes] and loss [batch] (None: not requested) of the device against
    float64 softmax cross-entropy of the fp32 logits z."""
    g, ref_loss = bc.xent_reference(z, labels)
    assert np.isfinite(dz).all()
    err = np.abs(dz.astype(np.float64) * rows - g).max()
    print(f"\n[measure] {what} max |dZ rows - ref| {err:.3e}")
    assert err <= DZ_ABS_CAP
    if loss is not None:
        rel = np.abs(loss - ref_loss) / np.maximum(np.abs(ref_loss), 1e-300)
        print(f"[measure] {what} loss rel err {rel.max():.3e}")
        assert loss == pytest.approx(ref_loss, rel=LOSS_REL, abs=0)


@pytest.mark.parametrize("i", range(len(bc.XENT_CASES)), ids=lambda i: str(bc.XENT_CASES[i]))
def test_xent_epilogue(cuda, monkeypatch, i):
    """BIAS_XENT: dZ and the mean loss from the exact logits, up to the documented limits
    M = 64 and N = 64, rows of logits spread over +-80 / +-90, labels in lane 0 and lane N - 1;
    loss = NULL is accepted and changes nothing else."""
    _set_shape(monkeypatch, None)
    c = bc.XENT_CASES[i]
    p = bc.xent_problem(c, seed=100 + i)
    z = p.oracle()[0]
    lab = p.labels[:, :c.M]
    assert (lab == 0).any() and (c.M == 1 or (lab == c.N - 1).any())
    dz, _, loss = run_twice(p, cuda)
    _check_xent(dz, loss, z, lab, c.M, str(c))
    c_noloss, _, none = run_bgemm(p, cuda, with_loss=False)
    assert none is None
    assert p.C.padding_intact(c_noloss)
    _same_bits(p.C.logical(c_noloss), dz, "dZ with loss = NULL")


def run_xent_grad(Zp, labels, Dp, cuda, with_loss=True):
    from distributed_learning_amd import _lib
    lib = _lib.load()
    batch, rows, classes = Zp.batch, Zp.rows, Zp.width
    Z, D, y = _dev(Zp.buf, cuda), _dev(Dp.buf, cuda), _dev(labels, cuda)
    loss = torch.from_numpy(np.full(batch + 4, bc.SENTINEL, np.uint32).view(np.float32)
                            ).to(cuda) if with_loss else None
    _lib.check(lib.dl_xent_grad(_lib.ptr(Z), Zp.stride, _lib.ptr(y), labels.shape[1],
                                _lib.ptr(D), Dp.stride, _lib.ptr(loss), batch, rows, classes,
                                _lib.stream_handle(cuda)), "dl_xent_grad")
    torch.cuda.synchronize()
    return D.cpu().numpy(), loss.cpu().numpy() if with_loss else None


@pytest.mark.parametrize("i", range(len(bc.XENT_GRAD_CASES)),
                         ids=lambda i: str(bc.XENT_GRAD_CASES[i]))
def test_xent_grad(cuda, monkeypatch, i):
    """dl_xent_grad (BatchedANN's head when the batch exceeds 64 rows): padded sZ / sY / sD,
    float64 reference, determinism, loss = NULL, and -- up to 64 rows -- the very bits of
    dl_bgemm's BIAS_XENT epilogue on the same logits (both call xent_row)."""
    _set_shape(monkeypatch, None)
    c = bc.XENT_GRAD_CASES[i]
    Z, lab = bc.xent_grad_logits(c, seed=200 + i)
    Zp = bc.Padded(c.batch, c.rows, c.classes, 0, Z)            # rows are dense: ld = classes
    Dp = bc.Padded(c.batch, c.rows, c.classes, 0, tail=7)
    labels = np.full((c.batch, c.rows + 2), -1, np.int32)
    labels[:, :c.rows] = lab
    d1, l1 = run_xent_grad(Zp, labels, Dp, cuda)
    d2, l2 = run_xent_grad(Zp, labels, Dp, cuda)
    assert np.array_equal(_bits(d1), _bits(d2)) and np.array_equal(_bits(l1), _bits(l2))
    assert Dp.padding_intact(d1) and np.all(_bits(l1)[c.batch:] == bc.SENTINEL)
    dz, loss = Dp.logical(d1).copy(), l1[:c.batch].copy()
    _check_xent(dz, loss, Z, lab, c.rows, str(c))
    d3, _ = run_xent_grad(Zp, labels, Dp, cuda, with_loss=False)
    assert np.array_equal(_bits(d3), _bits(d1))
    if c.rows <= 64:
        # z = Z . I + nothing: every fma of the chain adds an exact zero or Z itself
        eye = np.tile(np.eye(c.classes, dtype=np.float32), (c.batch, 1, 1))
        plab = np.full((c.batch, c.rows + 2), -1, np.int32)
        plab[:, :c.rows] = lab
        p = bc.Problem(c.rows, c.classes, c.classes, c.batch, 0, 0, "bias_xent", Z, eye,
                       labels=plab, want_loss=True)
        assert np.array_equal(p.oracle()[0], Z)
        gdz, _, gloss = run_twice(p, cuda)
        _same_bits(gdz, dz, "dZ of dl_bgemm BIAS_XENT against dl_xent_grad")
        _same_bits(gloss, loss, "loss of dl_bgemm BIAS_XENT against dl_xent_grad")
