"""A plain numpy model of the arithmetic of dl_mlp_grad / dl_mlp_eval (csrc/mlp_fused.hip): which
GEMMs of the ANNModel pass run as "bf16x6" and what that split computes.  A helper, not collected.

bf16x6: every fp32 operand is split exactly into three bf16 pieces x = h + m + l, and a product
a b keeps the six piece products that reach 2^-16 |a b|:  hh  +  (hm + mh + hl + lh + mm).  The
kernel sums hh in one fp32 accumulator and the five smaller terms in a second one that is added
at the end (mfma_x6, mfma32_x6); ``gemm(..., "x6")`` has that layout.  The degraded modes are the
kernels this model exists to tell apart from the real one: one small term lost ("no_mm": am bm,
"no_lh": al bh) or only hh + hm + mh kept ("x3").

In ``gemm(a, b, mode)`` the operand ``a`` is the kernel's A operand (the LDS-resident activation
or dZ, for dW1 the transposed dZ1) and ``b`` its B operand (the staged weight planes, for dW1 the
x chunk planes), so "al bh" means the same product here and there.

X6_GEMMS, where each was read in mlp_fused_kernel (the rest run on the fp32 MFMA):
  l1   layer 1: the ``if constexpr (L1X6)`` branch under "---- layer 1", mfma_x6 on the x and
       W1 planes (layer1_forward is the same code for mlp_eval_kernel);
  l2, l3   forward_hidden_all<L1X6> for layers 2 and 3 -> mma_x6_rows64 -> mfma_x6;
  dz2, dz1  backward_dz_all<L1X6> (dZ2 into H2, dZ1 into H1) -> mma_x6_rows64;
  dw1  the ``else if constexpr (L1X6)`` branch under "---- dW1", mfma32_x6; db1 is the ones
       column of x in the same tiles, so it takes the GEMM's mode too.
On the fp32 MFMA: the logits (mfma4 against the W4 image), dW4 / db4 (mfma4), dZ3
(backward_dz_one -> mma_rows64), dW3 / db3 and dW2 / db2 (weight_grad_hidden: mfma32 / mfma4;
"the hidden dW tiles stay on the fp32 MFMA").  Bias gradients ride in the weight-gradient GEMMs
as a ones column of the input operand, here as there.

The model's fp32 accumulation is numpy's sgemm, not the MFMA's order: it predicts the size of
the error, not its bits."""
import numpy as np

MODES = ("f64", "f32", "x6", "no_mm", "no_lh", "x3")
DEGRADED = ("no_mm", "no_lh", "x3")
GEMMS = ("l1", "l2", "l3", "l4", "dw4", "dz3", "dw3", "dz2", "dw2", "dz1", "dw1")
X6_GEMMS = ("l1", "l2", "l3", "dz2", "dz1", "dw1")
BLOCKS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias",
          "fc4.weight", "fc4.bias")

# the (a piece, b piece) products of the small accumulator, in the kernel's issue order
_SMALL = {"x6": ("lh", "hl", "mm", "mh", "hm"), "no_mm": ("lh", "hl", "mh", "hm"),
          "no_lh": ("hl", "mm", "mh", "hm"), "x3": ("mh", "hm")}


def mode_map(split="x6", rest="f32"):
    """GEMM name -> mode: ``split`` for the GEMMs the kernel runs split, ``rest`` for the others."""
    return {g: (split if g in X6_GEMMS else rest) for g in GEMMS}


def bf16_round(x):
    """fp32 -> nearest bf16 (ties to even) on the bit pattern, returned as fp32.  Finite inputs
    whose rounding stays finite."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split3(x):
    """(h, m, l) = (bf16(x), bf16(x - h), bf16(x - h - m)) as fp32 arrays; both differences are
    exact in fp32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = bf16_round(x)
    r = x - h
    m = bf16_round(r)
    return h, m, bf16_round(r - m)


def gemm(a, b, mode, acc=np.float32):
    """a [M, K] @ b [K, N] of fp32 values in ``mode``; "f64" returns float64, every other mode
    float32.  ``acc`` is the accumulator type of the split modes (float64: the split's own
    truncation error without any summation rounding)."""
    if mode == "f64":
        return a.astype(np.float64) @ b.astype(np.float64)
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if mode == "f32":
        return a @ b
    pa = dict(zip("hml", (p.astype(acc) for p in split3(a))))
    pb = dict(zip("hml", (p.astype(acc) for p in split3(b))))
    big = pa["h"] @ pb["h"]
    small = np.zeros_like(big)
    for t in _SMALL[mode]:
        small = small + pa[t[0]] @ pb[t[1]]
    return (big + small).astype(np.float32 if acc is np.float32 else acc)


def unflatten(flat, dims):
    """One agent's flat parameter row -> [(W, b)] of the four layers (the Mixer flatten order)."""
    din, dh, dout = dims
    out, off = [], 0
    for rows, cols in ((dh, din), (dh, dh), (dh, dh), (dout, dh)):
        W = flat[off:off + rows * cols].reshape(rows, cols)
        off += rows * cols
        out.append((W, flat[off:off + rows]))
        off += rows
    assert off == flat.size
    return out


def _forward(flat, x, dims, modes):
    f64 = all(modes[g] == "f64" for g in ("l1", "l2", "l3", "l4"))
    dt = np.float64 if f64 else np.float32
    (W1, b1), (W2, b2), (W3, b3), (W4, b4) = unflatten(flat, dims)
    z1 = gemm(x, W1.T, modes["l1"]).astype(dt) + b1.astype(dt)
    h1 = np.maximum(z1, 0)
    h2 = np.tanh(gemm(h1, W2.T, modes["l2"]).astype(dt) + b2.astype(dt))
    z3 = gemm(h2, W3.T, modes["l3"]).astype(dt) + b3.astype(dt)
    h3 = np.where(z3 > 0, z3, np.expm1(np.minimum(z3, 0)))
    z4 = gemm(h3, W4.T, modes["l4"]).astype(dt) + b4.astype(dt)
    return z1, h1, h2, h3, z4


def logits(flat, x, dims, modes):
    """The forward alone: [rows, dout]."""
    return _forward(flat, x, dims, modes)[4]


def grad_pass(flat, x, labels, dims, modes):
    """Forward + mean cross-entropy + backward of one agent: (flat gradient in the Mixer order,
    loss, z1, logits).  flat, x fp32; labels integer [rows].  With every mode "f64" the whole
    pass is float64; otherwise everything between the GEMMs is fp32."""
    dt = np.float64 if all(modes[g] == "f64" for g in GEMMS) else np.float32
    (W1, _), (W2, _), (W3, _), (W4, _) = unflatten(flat, dims)
    z1, h1, h2, h3, z4 = _forward(flat, x, dims, modes)
    B = x.shape[0]
    zs = z4 - z4.max(1, keepdims=True)
    e = np.exp(zs)
    s = e.sum(1, keepdims=True)
    rows = np.arange(B)
    loss = (np.log(s[:, 0]) - zs[rows, labels]).astype(np.float64).mean()
    dz4 = e / s
    dz4[rows, labels] -= 1
    dz4 = (dz4 / dt(B)).astype(dt)
    ones = np.ones((B, 1), dtype=np.float32)

    def wgrad(dz, hin, name):   # [dW | db] = dZ^T [Hin | 1]
        return gemm(dz.T, np.concatenate([hin.astype(dz.dtype), ones.astype(dz.dtype)], 1),
                    modes[name]).astype(dt)
    g4 = wgrad(dz4, h3, "dw4")
    dz3 = (gemm(dz4, W4, modes["dz3"]).astype(dt) * np.where(h3 > 0, dt(1), h3 + dt(1))).astype(dt)
    g3 = wgrad(dz3, h2, "dw3")
    dz2 = (gemm(dz3, W3, modes["dz2"]).astype(dt) * (dt(1) - h2 * h2)).astype(dt)
    g2 = wgrad(dz2, h1, "dw2")
    dz1 = (gemm(dz2, W2, modes["dz1"]).astype(dt) * (h1 > 0)).astype(dt)
    g1 = wgrad(dz1, x, "dw1")
    flat_g = np.concatenate([np.concatenate([g[:, :-1].reshape(-1), g[:, -1]])
                             for g in (g1, g2, g3, g4)])
    return flat_g, loss, z1, z4


def block_slices(dims):
    """Block name -> slice of the flat parameter row."""
    din, dh, dout = dims
    out, off = {}, 0
    for name, n in zip(BLOCKS, (dh * din, dh, dh * dh, dh, dh * dh, dh, dout * dh, dout)):
        out[name] = slice(off, off + n)
        off += n
    return out


# ---- the cap rule of tests/test_mlp_x6_gpu.py: err <= FACTOR * max(err_yardstick, 2^-23 scale)
FACTOR = 3.0
FLOOR = 2.0 ** -23


def cap(err_yardstick, scale, factor=FACTOR):
    return factor * max(float(err_yardstick), FLOOR * float(scale))
