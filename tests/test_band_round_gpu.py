"""GPU parity of the banded round (dl_band_round) with dl_mix_round's rule: bit for bit the oracle's
mix (oracle.cref.mix_round) of the numpy fp32 local step x - lr g, on graphs cut into several
blocks by small windows."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from oracle import cref
from test_band_blocks import banded, ring, torus
from test_sgd_round_gpu import dev_t, same

pytestmark = pytest.mark.gpu
LR = np.float32(0.05)
GRAPHS = {"ring": (lambda: ring(300), 48), "torus": (lambda: torus(12, 25), 60),
          "banded": (lambda: banded(300), 48)}


def E():
    from distributed_learning_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def problem(name, P, T):
    """(csr, band plan, X, G, W (X - lr G), W X): built once, shared, never modified."""
    from distributed_learning_amd.graph import band_blocks
    make, cap = GRAPHS[name]
    csr = make()
    plan = band_blocks(csr, cap, tile_cols=T, max_amplification=8.0)
    assert plan.blocks > 3
    rng = np.random.default_rng(P + len(name))
    X, G = (rng.standard_normal((csr.n_rows, P), dtype=np.float32) for _ in range(2))
    want = [cref.mix_round(S, csr.rowptr, csr.col, csr.w) for S in (X - LR * G, X)]
    for a in (X, G, *want):
        a.setflags(write=False)
    return csr, plan, X, G, want[0], want[1]


def padded(a, ld, cuda, fill=-7.5):
    buf = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=cuda)
    view = buf[:, :a.shape[1]]
    view.copy_(dev_t(a, cuda))
    return buf, view


# P = 256 in 4-column tiles: workgroups walk several tiles of a block; 37: a ragged last tile
@pytest.mark.parametrize("layout", ["rows", "rows_unaligned", "tiled"])
@pytest.mark.parametrize("with_g", [True, False])
@pytest.mark.parametrize("P,T", [(64, 16), (256, 4), (37, 8)])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_bits_match_the_oracle(cuda, name, P, T, with_g, layout):
    csr, plan, X, G, want_g, want_x = problem(name, P, T)
    want = want_g if with_g else want_x
    if layout == "tiled":
        g = E().GossipEngine(csr, P, device=cuda, X=dev_t(X, cuda), layout="tiled", tile_cols=T,
                             band=plan)
        assert g.band_plan is plan and g.layout == "tiled"
        g.round_band(g.layout_like(dev_t(G, cuda)) if with_g else None, float(LR))
        same(g.rows().cpu().numpy(), want, "rows()")
        return
    W, band = E().DeviceCsr(csr, cuda), E().DeviceBand(plan, cuda)
    ld = (P + 7) // 4 * 4 + (layout == "rows_unaligned")    # float4 tiles + a guarded tail; guarded
    (xb, x), (yb, y), (gb, g) = (padded(a, ld, cuda) for a in (X, 0 * X, G))
    if name == "torus" and P == 256:
        info = E().band_round_plan(W, band, x, y, g)
        assert info["n_items"] > info["grid"] and info["lds_bytes"] <= 160 * 1024
    E().band_round(W, band, x, y, g if with_g else None, float(LR))
    torch.cuda.synchronize()
    same(y.cpu().numpy(), want, "y")
    assert torch.equal(x, dev_t(X, cuda)) and torch.equal(g, dev_t(G, cuda))
    for b in (xb, yb, gb):
        assert torch.all(b[:, P:] == -7.5), "the padding past n_params was written"


@pytest.mark.parametrize("layout", ["rows", "tiled"])
def test_a_ring_beyond_the_tile_kernel(cuda, layout):
    """12 000 agents x 64: today's gather path (plan path 2); row-major through the engine's own
    plan, column-tiled (refused without a plan) with band=."""
    from distributed_learning_amd.graph import band_blocks
    n, P = 12000, 64
    csr = ring(n)
    rng = np.random.default_rng(12)
    X, G = (rng.standard_normal((n, P), dtype=np.float32) for _ in range(2))
    kw = dict(layout="tiled", tile_cols=16, band=band_blocks(csr)) if layout == "tiled" else \
        dict(layout="rows")
    g = E().GossipEngine(csr, P, device=cuda, X=dev_t(X, cuda), **kw)
    assert E().plan_shape(g.W, P)["path"] == 2 and g.band_plan.blocks > 1
    assert g.band_plan.amplification < 1.01
    g.round_band(g.layout_like(dev_t(G, cuda)), float(LR), deviation=layout == "rows")
    S, w, acc = X - LR * G, csr.w.astype(np.float32)[:3], np.zeros((n, P), np.float32)
    for k in range(3):
        acc = acc + w[k] * S[csr.col[k::3]]
    same(g.rows().cpu().numpy(), acc, "rows()")
    if layout == "tiled":     # (dl_deviation_tiled stages all agents: refused at this size)
        return
    dev = np.linalg.norm(acc.astype(np.float64) - acc.astype(np.float64).mean(0), axis=1)
    assert np.allclose(np.sqrt(g.dev_sq.cpu().numpy()), dev, rtol=1e-5)


def test_refusals(cuda):
    csr, plan, X, G, _, _ = problem("ring", 64, 16)
    W, x = E().DeviceCsr(csr, cuda), dev_t(X, cuda)
    buf = torch.zeros(2 * x.numel(), device=cuda)
    with pytest.raises(ValueError, match="y overlaps x"):
        E().band_round(W, E().DeviceBand(plan, cuda), buf[:x.numel()].view_as(x),
                       buf[64:64 + x.numel()].view_as(x))
    wide = dataclasses.replace(plan, max_window_rows=20000)
    with pytest.raises(ValueError, match="exceeds the LDS budget"):
        E().band_round(W, E().DeviceBand(wide, cuda), x, torch.empty_like(x))
    with pytest.raises(ValueError, match="does not fit the LDS tile kernel"):
        E().GossipEngine(ring(12000), 64, device=cuda, layout="tiled")
