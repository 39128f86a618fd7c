"""The Adam definition (adam_oracle.py, what dl_adam_step and dl_adam_round compute bit for bit)
against torch.optim.Adam / AdamW on the CPU, and the step count's recurrence against 1 - beta**t.

The bound on the definition's error is measured, not fixed in advance: over 20 steps on 64 x 777
with per-step gradient scales drawn from 1e-6 to 10, the definition's max absolute distance from
torch's fp64 run on the same inputs may be at most twice torch fp32's own distance from that run.
Measured (printed by the test): ratio 1.00 for all three option sets -- distances 1.25e-6
(plain), 9.9e-7 (L2 weight decay 5e-4), 3.9e-6 (decoupled weight decay 1e-2), torch fp32's the
same to three digits."""
import functools

import numpy as np
import pytest
import torch

import adam_oracle as O

N, P, STEPS, LR = 64, 777, 20, 1e-2
OPTS = {"plain": dict(weight_decay=0.0, decoupled=False),
        "l2": dict(weight_decay=5e-4, decoupled=False),
        "decoupled": dict(weight_decay=1e-2, decoupled=True)}


@functools.lru_cache(maxsize=None)
def inputs():
    """(X0, [G per step]): built once, shared, never modified."""
    rng = np.random.default_rng(20)
    X0 = rng.standard_normal((N, P), dtype=np.float32)
    scales = 10.0 ** rng.uniform(-6.0, 1.0, STEPS)
    Gs = [(rng.standard_normal((N, P)) * s).astype(np.float32) for s in scales]
    for a in [X0] + Gs:
        a.setflags(write=False)
    return X0, Gs


def torch_run(dtype, weight_decay, decoupled):
    X0, Gs = inputs()
    x = torch.from_numpy(np.array(X0)).to(dtype).requires_grad_(True)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([x], lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay, foreach=False)
    for G in Gs:
        x.grad = torch.from_numpy(np.array(G)).to(dtype)
        opt.step()
    return x.detach().double().numpy()


def oracle_run(weight_decay, decoupled):
    X, Gs = inputs()
    M, V, c = np.zeros_like(X), np.zeros_like(X), O.Coefs(LR)
    for G in Gs:
        c.tick()
        X, M, V = O.adam_step(X, G, M, V, LR, c.step_size, c.bias2_sqrt,
                              weight_decay=weight_decay, decoupled=decoupled)
    return X.astype(np.float64)


@pytest.mark.parametrize("name", list(OPTS))
def test_definition_is_as_close_to_fp64_as_torch_fp32(name):
    opt = OPTS[name]
    ref = torch_run(torch.float64, **opt)
    d_torch = float(np.max(np.abs(torch_run(torch.float32, **opt) - ref)))
    d_oracle = float(np.max(np.abs(oracle_run(**opt) - ref)))
    print(f"adam host [{name}]: |oracle - fp64| = {d_oracle:.3e}, |torch fp32 - fp64| = "
          f"{d_torch:.3e}, ratio {d_oracle / d_torch:.2f}")
    assert d_torch > 0.0
    assert d_oracle <= 2.0 * d_torch


@pytest.mark.parametrize("t", [1, 2, 10, 1000])
def test_recurrence_matches_the_powers(t):
    """The running products of the host mirror (engine.AdamState) and of the oracle are 1 -
    beta**t to 1e-15 relative, and the two follow each other bit for bit."""
    from distributed_learning_amd.engine import AdamState
    lr, betas = 3e-3, (0.9, 0.999)
    s, c = AdamState(lr, betas), O.Coefs(lr, betas)
    for _ in range(t):
        s.advance_host()
        c.tick()
    assert s.t == c.t == t
    for got, beta in ((s.b1t, betas[0]), (s.b2t, betas[1])):
        assert abs((1.0 - got) - (1.0 - beta ** t)) <= 1e-15 * (1.0 - beta ** t)
    assert (s.b1t, s.b2t) == (c.b1t, c.b2t)
    assert s.step_size.tobytes() == c.step_size.tobytes()
    assert s.bias2_sqrt.tobytes() == c.bias2_sqrt.tobytes()
    assert s.step_size == np.float32(lr / (1.0 - s.b1t))
