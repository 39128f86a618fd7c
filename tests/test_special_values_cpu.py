"""The special-value inputs of tests/special_values.py, checked on the CPU alone: the C oracle
equals the reference's Python fold (utils/consensus_simple/mixer.py:47) under ``same_bits`` on
NaN, infinities, subnormals and signed zeros; the inputs of every shape the GPU tests run keep
the properties that make a comparison meaningful (a comparison cannot pass on an all-NaN
matrix); a deviation's class (finite, inf, NaN) does not depend on the order the column mean is
summed in; and the host's one stop-rule decision (stop_rule.below_eps)."""
import numpy as np
import pytest

import special_values as sv
from oracle import cref
from oracle import mixer_ref as M

ROUNDS = 3   # dl_mix_rounds / dl_mix_rounds_trace / dl_mix_until run three rounds in the GPU tests


def oracle_round(case, stepped):
    with np.errstate(all="ignore"):
        return cref.mix_round(case.X, case.csr.rowptr, case.csr.col, case.csr.w,
                              G=case.G if stepped else None, lr=case.lr if stepped else 0.0)


def test_same_bits_comparator():
    f = np.float32
    nan2 = np.uint32(0xFFC00123).view(f)     # another sign and payload
    assert sv.same_bits([f("nan"), 1.0, -0.0, f("inf")], [nan2, 1.0, -0.0, f("inf")])
    assert not sv.same_bits([0.0], [-0.0])
    assert not sv.same_bits([f("inf")], [f("-inf")])
    assert not sv.same_bits([1.0], [f("nan")])
    assert not sv.same_bits([f("nan")], [1.0])
    assert not sv.same_bits([sv.MIN_SUB], [0.0])
    assert sv.mismatches([0.0, 1.0], [-0.0, 1.0]).tolist() == [True, False]


def test_ring_8x37_counts():
    """The 8 x 37 ring the agreement was first seen on: the fold of special values really
    produces NaN and subnormal outputs."""
    from distributed_learning_amd.graph import Csr
    n = 8
    cl = np.concatenate([[a, (a + 1) % n, (a - 1) % n] for a in range(n)])
    csr = Csr(np.arange(0, 3 * n + 1, 3), cl, np.tile([0.5, 0.3, 0.2], n))
    nan = sub = 0
    for cls in sv.CLASSES:
        case = sv.build(cls, n, 37, csr, zero=True)
        with np.errstate(all="ignore"):
            want = M.mix_once(case.X, case.csr.rowptr, case.csr.col, case.csr.w)
        got = oracle_round(case, False)
        assert sv.same_bits(got, want), (cls, sv.describe(got, want))
        nan += int(np.isnan(want).sum())
        sub += int(((np.abs(want) > 0) & (np.abs(want) < sv.MIN_NORM)).sum())
    assert nan >= 4 and sub >= 8, (nan, sub)


@pytest.mark.parametrize("cls", sv.CLASSES)
@pytest.mark.parametrize("name", sorted(sv.SHAPES))
def test_c_oracle_equals_the_python_fold(name, cls):
    """cref.mix_round (C, -ffp-contract=off -fno-fast-math) against sum(X[nbr] * w for ...) in
    numpy fp32, plain and with the local step in front, one round and three."""
    case = sv.shape_case(name, cls)
    rp, cl, w = case.csr.rowptr, case.csr.col, case.csr.w
    with np.errstate(all="ignore"):
        want = M.mix_once(case.X, rp, cl, w)
        got = cref.mix_round(case.X, rp, cl, w)
        assert sv.same_bits(got, want), sv.describe(got, want)
        want_s = M.mix_once(M.sgd_step(case.X, case.G, case.lr), rp, cl, w)
        got_s = cref.mix_round(case.X, rp, cl, w, G=case.G, lr=case.lr)
        assert sv.same_bits(got_s, want_s), sv.describe(got_s, want_s)
        for _ in range(ROUNDS - 1):
            want, got = M.mix_once(want, rp, cl, w), cref.mix_round(got, rp, cl, w)
        assert sv.same_bits(got, want), sv.describe(got, want)


@pytest.mark.parametrize("cls", sv.CLASSES)
@pytest.mark.parametrize("name", ["small_8x37", "rows_64x256", "rounds_100x1024", "until_3x1"])
def test_oracle_column_mean_equals_numpy(name, cls):
    """oracle.mixer_ref.column_mean and cref.column_mean against np.mean(axis=0) and
    np.add.reduce (mixer.py:61) on the inputs and on a round's output: the rows are added in
    order from +0.0, so a column of -0.0 has the mean +0.0."""
    case = sv.shape_case(name, cls)
    with np.errstate(all="ignore"):
        for A in (case.X, oracle_round(case, True)):
            want = np.mean(A, axis=0)
            assert sv.same_bits(np.add.reduce(A, axis=0) / np.float32(A.shape[0]), want)
            assert sv.same_bits(M.column_mean(A), want), sv.describe(M.column_mean(A), want)
            assert sv.same_bits(cref.column_mean(A), want), sv.describe(cref.column_mean(A), want)
    if cls == "tiny" and case.X.shape[1] >= 8:
        c = sv.feature_columns(case.X.shape[1], 5)[1]
        assert (sv.bits(case.X[:, c]) == 0x80000000).all() and sv.bits(M.column_mean(case.X))[c] == 0


def subnormal(v):
    return (np.abs(v) > 0) & (np.abs(v) < sv.MIN_NORM)


@pytest.mark.parametrize("cls", sv.CLASSES)
@pytest.mark.parametrize("name", sorted(sv.SHAPES))
def test_inputs_keep_their_conditions(name, cls):
    """On the oracle's round output alone: at most a quarter NaN; ``nonfinite`` has a NaN, a
    +inf and a -inf; ``tiny`` has a subnormal; the stepped matrix of ``tiny`` (what dl_sgd_step,
    dl_step_rows and dl_axpby return, and what the fused rounds fold) has a -0.0.  A fold from
    +0.0 cannot end in -0.0 (x + y is -0.0 only when both are), so a round's output has none and
    the -0.0 condition is on the stepped matrix.

    until_3x1 has three elements: one NaN is already more than a quarter, and one column holds
    one feature.  There the conditions that three elements can meet are checked: the class's
    first feature is present and the output is not all NaN."""
    case = sv.shape_case(name, cls)
    n, P = case.X.shape
    outs = [oracle_round(case, False), oracle_round(case, True)]
    with np.errstate(all="ignore"):
        stepped = M.sgd_step(case.X, case.G, case.lr)
    if n * P < 16:
        for Y in outs:
            assert not np.isnan(Y).all()
        assert {"tiny": subnormal(outs[0]).any(), "huge": np.abs(case.X).max() >= 2.0 ** 127,
                "nonfinite": np.isnan(outs[0]).any()}[cls]
        return
    for Y in outs:
        assert np.isnan(Y).sum() <= Y.size // 4, np.isnan(Y).sum()
        if cls == "nonfinite":
            assert np.isnan(Y).any() and np.isposinf(Y).any() and np.isneginf(Y).any()
        if cls == "tiny":
            assert subnormal(Y).any() and np.isfinite(Y).all()
    if cls == "tiny":
        assert (sv.bits(stepped) == 0x80000000).any()
        assert np.isfinite(sv.dev_sq32(outs[0])).all() and np.isfinite(sv.dev_sq32(outs[1])).all()
    if cls == "huge":
        assert np.isinf(stepped).any() and not np.isinf(case.X).any()
    if cls == "nonfinite" and sv.SHAPES[name][3]:
        # the 0.0-weight entry meets the +inf: numpy's 0 * inf
        h, c = sv.inf_agent(case.csr), sv.feature_columns(P, 4)[1]
        rows = np.repeat(np.arange(n), np.diff(case.csr.rowptr))
        hit = [int(rows[e]) for e in np.flatnonzero((case.csr.col == h) & (case.csr.w == 0.0))]
        assert hit and all(np.isnan(outs[0][q, c]) for q in hit)


def tree_mean(Y):
    """The column mean with the rows summed pairwise (halving), as a tree reduction does."""
    rows = [Y[r] for r in range(Y.shape[0])]
    while len(rows) > 1:
        nxt = [rows[i] + rows[i + 1] for i in range(0, len(rows) - 1, 2)]
        if len(rows) % 2:
            nxt.append(rows[-1])
        rows = nxt
    return rows[0] / np.float32(Y.shape[0])


@pytest.mark.parametrize("cls", ["huge", "nonfinite"])
@pytest.mark.parametrize("name", sorted(sv.SHAPES))
def test_deviation_class_is_independent_of_the_mean_order(name, cls):
    """Each agent's deviation about numpy's row-order mean (cref.deviation_sq) and about a mean
    summed pairwise falls in the same class -- finite, inf or NaN -- for the plain and the
    stepped round's output and for each of three rounds: the kernels sum the mean as a tree, and
    the GPU tests hold them to the oracle's class.  An input that fails this is to be changed,
    not the test."""
    case = sv.shape_case(name, cls)
    rp, cl, w = case.csr.rowptr, case.csr.col, case.csr.w
    with np.errstate(all="ignore"):
        Ys = [oracle_round(case, True), oracle_round(case, False)]
        for _ in range(ROUNDS - 1):
            Ys.append(cref.mix_round(Ys[-1], rp, cl, w))
        for i, Y in enumerate(Ys):
            seq = sv.classes_of(sv.dev_sq32(Y))
            tree = sv.classes_of(sv.dev_sq32(Y, tree_mean(Y)))
            assert np.array_equal(seq, tree), (i, np.flatnonzero(seq != tree)[:8])
            assert np.array_equal(sv.classes_of(M.column_mean(Y)), sv.classes_of(tree_mean(Y)))


# ---------------------------------------------------------------- the host's stop-rule decision
def test_below_eps():
    from distributed_learning_amd.stop_rule import below_eps
    f = np.float32
    assert below_eps(f(0.5e-3), 1e-3, 1) is True
    assert below_eps(f(2e-3), 1e-3, 1) is False
    assert below_eps(f("inf"), 1e-3, 1) is False            # inf: just not below eps
    eps = 1e-3
    assert below_eps(f(eps), eps, 1) is False                # equal (in float32) is not below
    assert below_eps(f(eps), f(eps), 1) is False
    for nan in (f("nan"), float("nan"), -f("nan")):
        with pytest.raises(FloatingPointError, match=r"after round 7\b"):
            below_eps(nan, 1e-3, 7)
        with pytest.raises(FloatingPointError, match=r"after round 0\b"):
            below_eps(nan, f(1e-3), 0)
        assert below_eps(nan, None, 3) is True               # eps None: nothing is tested
    assert below_eps(None, None, 0) is True


def test_nan_keeping_maxima():
    import torch
    from distributed_learning_amd.stop_rule import nan_max, nan_max_bits_
    f = np.float32
    assert nan_max([f(1), f(3), f(2)]) == f(3)
    assert nan_max([f("inf"), f(3)]) == f("inf")
    for vals in ([f("nan"), f(1)], [f(1), f("nan")], [f(1), f("nan"), f("inf")]):
        assert np.isnan(nan_max(vals))
    # the integer order of the prepared bits is the float order with every NaN on top
    vals = [0.0, 1e-45, 1.0, 3e38, float("inf"), float("nan")]
    keys = [int(nan_max_bits_(torch.tensor([v], dtype=torch.float32))[0]) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    neg_nan = torch.tensor([0xFFC00000 - (1 << 32)], dtype=torch.int32).view(torch.float32)
    assert int(nan_max_bits_(neg_nan)[0]) > keys[4]
