"""The numpy model of the fused MLP kernels' bf16x6 GEMMs (tests/x6_model.py) on the CPU: the
split is exact, the three dropped piece products are at fp32 rounding level, and -- on the very
inputs of tests/test_mlp_x6_gpu.py -- the cap rule of that file passes the true six-term split and
fails a kernel that lost one small term.  The last is what lets the GPU tests fail: deleting one of
the five small-term products from mfma_x6 / mfma32_x6 is the model's "no_mm" / "no_lh"."""
import functools

import numpy as np
import pytest

import x6_cases as xc
import x6_model as xm


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _split_inputs():
    rng = np.random.default_rng(0)
    e = np.arange(-100, 101, dtype=np.float64)
    full = np.float32(2.0 - 2.0 ** -23)                    # all 24 significand bits set
    mags = (rng.uniform(1, 2, 4000) * 2.0 ** rng.integers(-100, 100, 4000)).astype(np.float32)
    return {
        "normals": rng.standard_normal(20000).astype(np.float32),
        "powers of two": np.concatenate([2.0 ** e, -(2.0 ** e)]).astype(np.float32),
        "1 +- 2^-23": np.array([1 + 2.0 ** -23, 1 - 2.0 ** -23, -1 - 2.0 ** -23,
                                -1 + 2.0 ** -23, 1 - 2.0 ** -24], dtype=np.float32),
        "24 bits set": (full * 2.0 ** e).astype(np.float32) * np.float32(-1) ** np.arange(e.size),
        "zeros": np.array([0.0, -0.0], dtype=np.float32),
        "2^-100 .. 2^100": np.concatenate([mags, -mags]),
    }


@pytest.mark.parametrize("name", list(_split_inputs()))
def test_split_is_exact(name):
    """h + m + l == x bit for bit, every piece is a bf16 value, and the pieces shrink by 2^-8."""
    x = _split_inputs()[name]
    h, m, l = xm.split3(x)
    for p in (h, m, l):
        assert p.dtype == np.float32 and np.all(_bits(p) & 0xFFFF == 0)
    s = (h + m) + l                                       # each partial sum is exact in fp32
    if name == "zeros":
        assert np.all(s == 0) and np.array_equal(_bits(h), _bits(x))
    else:
        assert np.array_equal(_bits(s), _bits(x))
        assert np.array_equal(h.astype(np.float64) + m + l, x.astype(np.float64))
    ax = np.abs(x.astype(np.float64))
    assert np.all(np.abs(x - h) <= 2.0 ** -8 * ax) and np.all(np.abs(m) <= 2.0 ** -8 * ax)
    assert np.all(np.abs(l) <= 2.0 ** -16 * ax)


def test_bf16_round_is_nearest_even():
    one = np.float32(1.0)
    ulp = 2.0 ** -7                                       # bf16 spacing in [1, 2)
    x = np.array([1 + ulp / 2, 1 + 3 * ulp / 2, 1 + ulp / 2 + 2.0 ** -23, 1 + ulp / 4,
                  -(1 + ulp / 2)], dtype=np.float32)
    want = np.array([one, 1 + 2 * ulp, 1 + ulp, one, -one], dtype=np.float32)
    assert np.array_equal(_bits(xm.bf16_round(x)), _bits(want))


def test_dropped_terms_are_at_fp32_level():
    """With float64 accumulation the six-term sum is within 2^-23 sum_k |a_k| |b_k| of the exact
    product: |m| <= 2^-8 |x| and |l| <= 2^-16 |x|, so |ml + lm + ll| <= (2 * 2^-24 + 2^-32) |ab|
    < 2^-23 |ab|.  (Observed: under 2^-24.)  One lost small term is 2^-16-level, far outside."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for M, K, N in ((64, 784, 150), (64, 52, 40), (150, 64, 97), (7, 4, 2)):
        a = rng.standard_normal((M, K)).astype(np.float32)
        b = (rng.uniform(-1, 1, (K, N)) / np.sqrt(K)).astype(np.float32)
        exact = xm.gemm(a, b, "f64")
        mag = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
        six = xm.gemm(a, b, "x6", acc=np.float64)
        ratio = float((np.abs(six - exact) / mag).max())
        worst = max(worst, ratio)
        assert ratio <= 2.0 ** -23
        for mode in xm.DEGRADED:
            lost = float((np.abs(xm.gemm(a, b, mode, acc=np.float64) - exact) / mag).max())
            assert lost > 2.0 ** -22, (mode, lost)
    print(f"six terms, fp64 accumulation: max error / sum |a||b| = {worst:.3e} "
          f"= 2^{np.log2(worst):.2f}")
    assert worst < 2.0 ** -24


def test_model_f64_pass_is_autograd():
    """The model's backward is the module's: its all-float64 pass against torch's float64 autograd
    on the GPU tests' inputs."""
    for dims in ((52, 40, 7), (4, 2, 2)):
        o = xc.grad_oracle(dims)
        for a in range(o["X"].shape[0]):
            g, loss, _, z = xm.grad_pass(o["X"][a].numpy(), o["data"][a].numpy(),
                                         o["labels"][a].numpy().astype(np.int64), dims,
                                         {k: "f64" for k in xm.GEMMS})
            w = o["G64"][a].numpy()
            assert np.abs(g - w).max() <= 1e-12 * np.abs(w).max()
            assert abs(loss - float(o["loss64"][a])) <= 1e-12
            assert np.abs(z - o["z64"][a].numpy()).max() <= 1e-12


def test_seed_tables_are_the_search_results():
    """The case tables hold what the search finds: the first seeds with a ReLU margin of 6 x the
    fp32 pre-activation error."""
    for dims, seeds in xc.GRAD_CASES.items():
        assert xc.search_seeds(dims, len(seeds)) == seeds, dims
    for dims, seeds in xc.LOGIT_CASES.items():
        assert xc.search_seeds(dims, len(seeds), rows=xc.LOGIT_ROWS) == seeds, dims


@functools.lru_cache(maxsize=None)
def _grad_ratios(dims):
    """mode -> block -> (largest over the agents of err / uncapped bound), the uncapped bound
    being max(err of the all-fp32 model, 2^-23 scale): the cap rule's right-hand side without
    its factor."""
    o = xc.grad_oracle(dims)
    n = o["X"].shape[0]
    args = [(o["X"][a].numpy(), o["data"][a].numpy(), o["labels"][a].numpy().astype(np.int64))
            for a in range(n)]
    yard = [xm.grad_pass(*args[a], dims, {g: "f32" for g in xm.GEMMS})[0] for a in range(n)]
    out = {}
    for mode in ("x6",) + xm.DEGRADED:
        got = [xm.grad_pass(*args[a], dims, xm.mode_map(mode))[0] for a in range(n)]
        out[mode] = {}
        for name, s in xm.block_slices(dims).items():
            r = 0.0
            for a in range(n):
                w = o["G64"][a].numpy()[s]
                base = xm.cap(np.abs(yard[a][s] - w).max(), np.abs(w).max(), factor=1.0)
                r = max(r, float(np.abs(got[a][s] - w).max()) / base)
            out[mode][name] = r
    return out


@functools.lru_cache(maxsize=None)
def _logit_ratios(dims):
    o = xc.logit_oracle(dims)
    x = o["data"].numpy()
    out = {}
    for mode in ("x6",) + xm.DEGRADED:
        r = 0.0
        for a in range(o["X"].shape[0]):
            f, w = o["X"][a].numpy(), o["z64"][a].numpy()
            yard = xm.logits(f, x, dims, {g: "f32" for g in xm.GEMMS})
            base = xm.cap(np.abs(yard - w).max(), np.abs(w).max(), factor=1.0)
            r = max(r, float(np.abs(xm.logits(f, x, dims, xm.mode_map(mode)) - w).max()) / base)
        out[mode] = r
    return out


@pytest.mark.parametrize("dims", list(xc.GRAD_CASES), ids=xc.case_id)
def test_gradient_cases_discriminate(dims):
    """On the GPU test's own inputs: the six-term model is within the cap on every block, and each
    degraded variant exceeds it on fc1.weight and on at least two other blocks.  A per-block
    factor (x6_cases.FACTORS) may never exceed half the smallest degraded ratio of its block."""
    r = _grad_ratios(dims)
    for name, v in r["x6"].items():
        print(f"{dims} {name}: x6 {v / xc.factor(dims, name):.2f} of the cap; lost terms "
              + ", ".join(f"{m} {r[m][name] / xc.factor(dims, name):.1f} x" for m in xm.DEGRADED))
        assert v <= xc.factor(dims, name), (dims, name, v)
    for mode in xm.DEGRADED:
        over = [name for name, v in r[mode].items() if v > xc.factor(dims, name)]
        assert "fc1.weight" in over and len(over) >= 3, (dims, mode, over)
    for (d, name), f in xc.FACTORS.items():
        if d == dims and name in xm.BLOCKS:
            assert f <= 0.5 * min(r[m][name] for m in xm.DEGRADED), (dims, name, f)


@pytest.mark.parametrize("dims", list(xc.LOGIT_CASES), ids=xc.case_id)
def test_logit_cases_discriminate(dims):
    r = _logit_ratios(dims)
    f = xc.factor(dims, "logits")
    print(f"{dims} logits: x6 {r['x6'] / f:.2f} of the cap; lost terms "
          + ", ".join(f"{m} {r[m] / f:.1f} x" for m in xm.DEGRADED))
    assert r["x6"] <= f
    for mode in xm.DEGRADED:
        assert r[mode] > f, (dims, mode, r[mode])
    if (dims, "logits") in xc.FACTORS:
        assert f <= 0.5 * min(r[m] for m in xm.DEGRADED)


def test_power_of_two_scaling_is_exact_in_the_model():
    """data * 2^s with fc1.weight * 2^-s: the model's split pass and its fp32 pass return the loss,
    the logits and every block but fc1.weight bit for bit, and fc1.weight's block times 2^s
    (dW1 = dZ1^T data carries the data's factor while dZ1 is unchanged) -- the property
    test_mlp_x6_gpu.py asserts of the kernels."""
    dims = (52, 40, 7)
    o = xc.grad_oracle(dims)
    f, x = o["X"][0].numpy().copy(), o["data"][0].numpy()
    y = o["labels"][0].numpy().astype(np.int64)
    w1 = xm.block_slices(dims)["fc1.weight"]
    for modes in (xm.mode_map("x6"), {g: "f32" for g in xm.GEMMS}):
        g0, l0, _, z0 = xm.grad_pass(f, x, y, dims, modes)
        for s in (32, -32):
            fs = f.copy()
            fs[w1] = np.ldexp(fs[w1], -s)
            g, l, _, z = xm.grad_pass(fs, np.ldexp(x, s), y, dims, modes)
            assert l == l0 and np.array_equal(_bits(z), _bits(z0))
            g[w1] = np.ldexp(g[w1], -s)
            assert np.array_equal(_bits(g), _bits(g0)), s
