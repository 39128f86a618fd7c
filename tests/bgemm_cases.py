"""Shared by tests/test_bgemm_ref_cpu.py and tests/test_bgemm_gpu.py: the dl_bgemm / dl_xent_grad
case lists, padded operand buffers, and the oracle / float64 references.

Every operand lives in a larger flat buffer: the row stride exceeds the logical width by 2,
3, 5 or 7 (never a multiple of 4) and the batch stride exceeds one batch's extent by 5.  Input
padding is NaN (a masked load that leaks padding poisons the result); output buffers are filled
with a NaN of a recognisable payload and everything outside the logical elements must come back
bit-unchanged.

Sizes cross each boundary of csrc/bgemm.hip: the 16-wide MFMA tile (15, 17), the 32 / 64 / 160
block tiles (63, 64, 65, 150, 161), the K slice BK = 32 (1, 3, 31, 32, 33, 64, 95) and the
8-XCD work-order remap (grids of fewer than 8 workgroups, exactly 8, and 9 / 12 / 81).
"""
import collections

import numpy as np

EPI = {"none": 0, "bias": 1, "bias_relu": 2, "bias_tanh": 3, "bias_elu": 4, "drelu": 5,
       "dtanh": 6, "delu": 7, "bias_xent": 8}
SENTINEL = np.uint32(0x7FC5A5A5)      # a quiet NaN no arithmetic here produces
U = 2.0 ** -24                        # fp32 unit roundoff

Case = collections.namedtuple(
    "Case", "M N K batch ta tb epi bias_null rowsum shape", defaults=(False, False, None))


def case_id(c):
    s = f"{c.M}x{c.N}x{c.K}b{c.batch}-{'t' if c.ta else 'n'}{'t' if c.tb else 'n'}-{c.epi}"
    if c.bias_null:
        s += "-nobias"
    if c.rowsum:
        s += "-rowsum"
    if c.shape is not None:
        s += f"-shape{c.shape}"
    return s


def grid_size(c, bm=64, bn=64):
    return -(-c.M // bm) * -(-c.N // bn) * c.batch


# Epilogues whose result is a rounded fp32 expression of the fma chain: C is compared bit for bit.
# 64 x 64 tiles unless a shape is named: grid sizes 1 (1x1x1 b1), 9 (b9 of one tile; 161x161 b1),
# 12 (65x65 b3), 81 (161x161 b9); shape 5 (16 x 64) on 63x65 b1 is exactly 8 workgroups.
LINEAR_CASES = [
    Case(1, 1, 1, 1, 0, 0, "none"),
    Case(1, 1, 1, 9, 1, 1, "bias"),
    Case(15, 17, 3, 3, 0, 1, "bias_relu"),
    Case(17, 15, 31, 1, 1, 0, "drelu"),
    Case(63, 64, 32, 1, 0, 0, "delu"),
    Case(64, 63, 33, 3, 1, 1, "none"),
    Case(64, 64, 64, 1, 0, 1, "bias"),
    Case(65, 65, 95, 3, 1, 0, "bias_relu"),
    Case(150, 150, 64, 1, 0, 1, "bias"),
    Case(161, 161, 95, 1, 0, 0, "none"),
    Case(161, 161, 95, 9, 1, 1, "delu"),
    Case(161, 1, 33, 3, 1, 0, "bias"),
    Case(1, 161, 32, 3, 0, 1, "drelu"),
    Case(17, 150, 95, 1, 1, 1, "bias_relu"),
    Case(65, 15, 1, 1, 0, 0, "bias", bias_null=True),
    Case(15, 65, 3, 9, 0, 1, "bias_relu", bias_null=True),
    Case(63, 63, 95, 1, 1, 1, "drelu"),
    Case(64, 64, 32, 9, 1, 0, "none"),
    Case(65, 64, 33, 1, 0, 0, "delu"),
    Case(64, 65, 31, 3, 0, 1, "none"),
    Case(150, 161, 1, 1, 1, 0, "bias"),
    Case(161, 150, 3, 3, 0, 0, "drelu"),
    Case(1, 17, 64, 1, 1, 1, "delu"),
    Case(17, 1, 95, 9, 0, 1, "none"),
    Case(63, 161, 64, 3, 1, 1, "bias"),
    Case(63, 65, 33, 1, 0, 1, "bias_relu", shape=5),      # exactly 8 workgroups
    # rowsum (written by tile_x == 0 only): ta 0 and 1, M over several tiles in y, N over
    # several tiles in x, and the 16- and 160-row tiles (one thread per tile row)
    Case(150, 17, 31, 9, 1, 0, "none", rowsum=True),
    Case(161, 150, 33, 3, 1, 0, "none", rowsum=True),
    Case(161, 65, 95, 1, 0, 1, "bias", rowsum=True),
    Case(17, 161, 31, 3, 0, 0, "none", rowsum=True),
    Case(65, 1, 64, 9, 1, 1, "none", rowsum=True),
    Case(150, 161, 3, 1, 1, 0, "drelu", rowsum=True),
    Case(63, 65, 33, 3, 1, 0, "none", rowsum=True, shape=5),
    Case(161, 161, 32, 1, 0, 0, "none", rowsum=True, shape=4),
    Case(161, 65, 1, 3, 1, 1, "none", rowsum=True, shape=2),
]

DTANH_CASES = [
    Case(63, 65, 33, 3, 0, 0, "dtanh"),
    Case(161, 17, 95, 1, 0, 1, "dtanh"),
    Case(1, 150, 3, 9, 1, 0, "dtanh"),
    Case(64, 64, 32, 1, 1, 1, "dtanh"),
]

ACT_CASES = [Case(*s, e) for e in ("bias_tanh", "bias_elu") for s in (
    (64, 150, 95, 3, 0, 1), (17, 161, 33, 1, 1, 0), (161, 15, 3, 9, 0, 0), (1, 1, 1, 1, 1, 1),
    (65, 63, 64, 1, 1, 1))] + [Case(15, 17, 31, 3, 0, 1, "bias_tanh", bias_null=True),
                               Case(63, 64, 32, 1, 0, 0, "bias_elu", bias_null=True)]

# (M, N, K, batch, ta, tb, spread 0 / 80 / 90): M in {1, 5, 63, 64}, N in {1, 2, 7, 63, 64}
XentCase = collections.namedtuple("XentCase", "M N K batch ta tb spread")
XENT_CASES = [
    XentCase(1, 1, 1, 1, 0, 0, 0),
    XentCase(5, 2, 3, 3, 0, 1, 0),
    XentCase(63, 7, 33, 9, 1, 0, 0),
    XentCase(64, 64, 95, 3, 1, 1, 0),
    XentCase(64, 63, 31, 1, 0, 1, 80),
    XentCase(1, 64, 64, 3, 0, 0, 90),
    XentCase(5, 63, 32, 1, 1, 1, 0),
    XentCase(63, 1, 3, 3, 1, 0, 0),
    XentCase(64, 2, 1, 9, 0, 1, 80),
    XentCase(5, 7, 95, 3, 0, 1, 90),
]

# (rows, classes, batch, spread): classes in {1, 2, 10, 63, 64}, rows in {1, 3, 4, 5, 65, 130}
XentGradCase = collections.namedtuple("XentGradCase", "rows classes batch spread")
XENT_GRAD_CASES = [
    XentGradCase(1, 1, 1, 0),
    XentGradCase(3, 2, 3, 80),
    XentGradCase(4, 10, 1, 0),
    XentGradCase(5, 63, 3, 90),
    XentGradCase(65, 64, 1, 0),
    XentGradCase(130, 10, 3, 80),
    XentGradCase(1, 64, 3, 90),
    XentGradCase(65, 2, 3, 0),
    XentGradCase(4, 1, 3, 0),
]

# tile shapes 0-5 x the four ta/tb pairs, each at one size per selector (M <= 64 / M > 64)
SHAPE_SIZES = [(63, 65, 33, 3, "bias_relu"), (161, 65, 31, 1, "delu")]


# ---------------------------------------------------------------------------- padded buffers
class Padded:
    """[batch][rows][width] logical values inside a flat fp32 buffer (row stride ld, batch stride
    `stride`), every other element `fill` (NaN, or the sentinel for outputs)."""

    def __init__(self, batch, rows, width, pad, values=None, tail=5):
        self.batch, self.rows, self.width = batch, rows, width
        self.ld = width + pad
        self.stride = rows * self.ld + tail
        self.buf = np.full(batch * self.stride + 3, np.nan, np.float32)
        if values is None:
            self.buf.view(np.uint32)[:] = SENTINEL
        else:
            self.logical(self.buf)[...] = values

    def logical(self, buf):
        """Writable [batch][rows][width] view of the logical elements of `buf`."""
        return np.lib.stride_tricks.as_strided(
            buf, (self.batch, self.rows, self.width),
            (4 * self.stride, 4 * self.ld, 4), writeable=True)

    def padding_intact(self, buf):
        """True when every element of `buf` outside the logical ones still holds the sentinel."""
        pad = np.ones(buf.shape, np.float32)
        self.logical(pad)[...] = 0
        return bool(np.all(buf.view(np.uint32)[pad != 0] == SENTINEL))


def _normal(rng, shape):
    """Normal-range fp32 values: |x| >= 2^-10, so no product of two underflows or is subnormal."""
    x = rng.standard_normal(shape).astype(np.float32)
    tiny = np.abs(x) < 2.0 ** -10
    x[tiny] = np.where(x[tiny] < 0, np.float32(-2.0 ** -10), np.float32(2.0 ** -10))
    return x


class Problem:
    """One dl_bgemm call: logical operands, their padded storage, and the argument values."""

    def __init__(self, M, N, K, batch, ta, tb, epi, opA, opB, bias=None, H=None, rowsum=False,
                 labels=None, want_loss=False):
        self.M, self.N, self.K, self.batch, self.ta, self.tb = M, N, K, batch, ta, tb
        self.epi = EPI[epi] if isinstance(epi, str) else epi
        self.opA, self.opB, self.bias_v, self.H_v = opA, opB, bias, H   # logical, fp32
        self.A = Padded(batch, K if ta else M, M if ta else K, 3,
                        opA.transpose(0, 2, 1) if ta else opA)
        self.B = Padded(batch, N if tb else K, K if tb else N, 5,
                        opB.transpose(0, 2, 1) if tb else opB)
        self.C = Padded(batch, M, N, 7)
        self.bias = Padded(batch, 1, N, 3, bias[:, None, :], tail=0) if bias is not None else None
        self.H = Padded(batch, M, N, 2, H) if H is not None else None
        self.rowsum = Padded(batch, 1, M, 3, tail=0) if rowsum else None
        self.labels = labels                     # int32 [batch][M + 2] (stride M + 2) or None
        self.want_loss = want_loss

    def oracle(self):
        """ref_bgemm on the padded host buffers -> (C, C2 or None, rowsum or None) logical
        arrays; checks that the oracle leaves the output padding alone."""
        from oracle import cref
        c = self.C.buf.copy()
        c2 = self.C.buf.copy() if self.epi == EPI["dtanh"] else None
        rs = self.rowsum.buf.copy() if self.rowsum else None
        cref.bgemm(self.batch, self.M, self.N, self.K, self.A.buf, self.A.ld, self.A.stride,
                   self.ta, self.B.buf, self.B.ld, self.B.stride, self.tb, c, self.C.ld,
                   self.C.stride, self.epi,
                   self.bias.buf if self.bias else None, self.bias.stride if self.bias else 0,
                   self.H.buf if self.H else None, self.H.ld if self.H else 0,
                   self.H.stride if self.H else 0, c2,
                   rs, self.rowsum.stride if self.rowsum else 0)
        assert self.C.padding_intact(c)
        assert c2 is None or self.C.padding_intact(c2)
        assert rs is None or self.rowsum.padding_intact(rs)
        return (self.C.logical(c).copy(), self.C.logical(c2).copy() if c2 is not None else None,
                self.rowsum.logical(rs)[:, 0, :].copy() if rs is not None else None)


def _activation_output(rng, epi, shape):
    """H as the forward pass leaves it, with the edge values of each activation planted."""
    z = _normal(rng, shape)
    flat = np.arange(z.size).reshape(shape)
    if epi == "drelu":
        return np.maximum(z, np.float32(0))                    # exact zeros and positives
    if epi == "dtanh":
        h = np.tanh(z.astype(np.float64)).astype(np.float32)
        h[flat % 11 == 0] = 1.0                                # saturated: 1 - h h = 0
        h[flat % 13 == 0] = -1.0
        h[flat % 17 == 0] = 0.0
        return h
    h = np.where(z > 0, 3 * z, np.expm1(3 * z.astype(np.float64))).astype(np.float32)
    h[flat % 11 == 0] = -1.0                                   # saturated ELU: h + 1 = 0
    h[flat % 13 == 0] = 0.0                                    # h > 0 is false at 0: h + 1 = 1
    return h


def linear_problem(c, seed):
    """Problem of a Case with one of the bit-defined epilogues (and BIAS_TANH / BIAS_ELU, whose
    oracle output is the pre-activation)."""
    rng = np.random.default_rng(seed)
    opA = _normal(rng, (c.batch, c.M, c.K))
    opB = _normal(rng, (c.batch, c.K, c.N))
    bias = H = None
    if c.epi in ("bias_tanh", "bias_elu"):
        # z around 0 at every scale down to 2^-12 of a unit, beside |z| large of both signs:
        # tanh -> +-1, ELU -> -1 and the identity branch
        opB = opB * (2.0 ** -(np.arange(c.N) % 13)).astype(np.float32)
        if not c.bias_null:
            pat = np.array([0, 0.5, -0.5, 0, 20, -20, -100, 100, 0, -8, 8], np.float32)
            bias = np.tile(pat[np.arange(c.N) % len(pat)], (c.batch, 1))
            bias[:, ::5] += _normal(rng, bias[:, ::5].shape) * np.float32(2.0 ** -6)
    elif c.epi.startswith("bias") and not c.bias_null:
        bias = _normal(rng, (c.batch, c.N))
    if c.epi in ("drelu", "dtanh", "delu"):
        H = _activation_output(rng, c.epi, (c.batch, c.M, c.N))
    return Problem(c.M, c.N, c.K, c.batch, c.ta, c.tb, c.epi, opA, opB, bias, H, c.rowsum)


def restored(p, ta, tb):
    """The same logical product with the operands stored the other way round."""
    return Problem(p.M, p.N, p.K, p.batch, ta, tb, p.epi, p.opA, p.opB, p.bias_v, p.H_v,
                   p.rowsum is not None)


# ---------------------------------------------------------------------------- cross-entropy
def xent_labels(rng, batch, rows, classes):
    """Rows with the label in lane 0, rows with it in lane classes - 1, the rest random."""
    lab = rng.integers(0, classes, (batch, rows)).astype(np.int32)
    lab[:, 0::3] = 0
    lab[:, 1::3] = classes - 1
    return lab


def spread_offsets(classes, amp):
    """Per-class offsets spanning -amp .. +amp within a row (amp 80, and 90: expf overflows past
    88.7, so there a softmax without the max subtraction gives inf / inf).  The largest sits in
    the middle lane (2 classes: lane 1), not in lane 0 where every batch has a planted label,
    so each batch's mean loss is of order ten."""
    if classes == 1:
        return np.zeros(1, np.float32)
    off = np.linspace(-float(amp), float(amp), classes).astype(np.float32)
    return np.roll(off, classes // 2 + 1) if classes > 2 else off


def xent_problem(c, seed, want_loss=True):
    rng = np.random.default_rng(seed)
    opA = _normal(rng, (c.batch, c.M, c.K))
    # logits of order one: the mean loss stays well above the fp32 resolution of
    # logsumexp(z) - z[label], which a relative tolerance presupposes
    opB = _normal(rng, (c.batch, c.K, c.N)) * np.float32(2.0 ** -np.ceil(np.log2(c.K) / 2))
    if c.spread:
        bias = np.tile(spread_offsets(c.N, c.spread), (c.batch, 1))
    else:
        bias = _normal(rng, (c.batch, c.N)) * np.float32(0.5)
    labels = np.full((c.batch, c.M + 2), -1, np.int32)
    labels[:, :c.M] = xent_labels(rng, c.batch, c.M, c.N)
    return Problem(c.M, c.N, c.K, c.batch, c.ta, c.tb, "bias_xent", opA, opB, bias,
                   labels=labels, want_loss=want_loss)


def xent_grad_logits(c, seed):
    """Z [batch][rows][classes] fp32 and labels [batch][rows] for dl_xent_grad."""
    rng = np.random.default_rng(seed)
    Z = _normal(rng, (c.batch, c.rows, c.classes))
    if c.spread:
        Z = Z + spread_offsets(c.classes, c.spread)
    return Z.astype(np.float32), xent_labels(rng, c.batch, c.rows, c.classes)


def xent_reference(z, labels):
    """float64 softmax cross-entropy of fp32 logits z [batch][rows][classes]:
    (dZ * rows = softmax - onehot, mean loss per batch)."""
    z = z.astype(np.float64)
    zs = z - z.max(axis=2, keepdims=True)
    e = np.exp(zs)
    s = e.sum(axis=2, keepdims=True)
    g = e / s
    b, r = np.indices(labels.shape)
    g[b, r, labels] -= 1.0
    loss = (np.log(s[..., 0]) - zs[b, r, labels]).mean(axis=1)
    return g, loss


def ulp_distance(got, ref64):
    """|got - ref| in units of the spacing of fp32 at the (rounded) reference."""
    ref32 = ref64.astype(np.float32)
    ulp = np.spacing(np.abs(ref32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - ref64) / ulp


def product_f64(p):
    """float64 op(A).op(B) and the magnitude sum  sum_k |a||b|  of a Problem."""
    a, b = p.opA.astype(np.float64), p.opB.astype(np.float64)
    return a @ b, np.abs(a) @ np.abs(b)
