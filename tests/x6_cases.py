"""Inputs and float64 oracles shared by tests/test_mlp_x6_gpu.py and tests/test_x6_model_cpu.py
(a helper, not collected; CPU only).

Every agent is the project's ``ANNModel`` with torch's default init under
``torch.manual_seed(seed)``; ``randn`` data and ``randint`` labels come from a CPU generator; the
oracle is the same module in ``.double()``, differentiated from the same fp32 values.

The ReLU is the only decision in this network: an fp32 pass whose z1 has another sign than the
fp64 one differs by a finite amount.  ``relu_margin`` measures how far the fp64 forward keeps from
that, and the seeds below were searched on the CPU with it: 0, 1, ... in order, the first ones
with min |z1| >= 6 x the largest |z1(fp32, CPU) - z1(fp64)| (the tests assert 4 x)."""
import functools

import torch
import torch.nn.functional as F

BATCH = 64
SEARCH_RATIO, ASSERT_RATIO = 6.0, 4.0

# gradient cases: dims -> one searched seed per agent (model, data and labels under that seed)
GRAD_CASES = {
    (784, 150, 10): (0, 1),     # c3's own shape
    (52, 40, 7): (0, 1),        # ragged last K slice
    (16, 152, 16): (0, 1),      # K under one 32-slice; widest hidden and head
    (4, 2, 2): (0, 1),          # every minimum at once
    (36, 34, 3): (0, 1),        # one slice + 4
    (4, 152, 16): (0, 1),       # minimum input, widest hidden
    (64, 2, 16): (0, 1),        # minimum hidden
}
# logits cases: LOGIT_ROWS shared rows (two full 64-row blocks and one of two rows) from
# Generator().manual_seed(LOGIT_DATA_SEED); dims -> one searched model seed per agent
LOGIT_ROWS, LOGIT_DATA_SEED = 130, 1
LOGIT_CASES = {
    (784, 150, 10): (2, 3),
    (52, 40, 7): (0, 1),
    (4, 2, 2): (0, 1),
    (16, 152, 16): (0, 1),
}
# cases of the scaling and the all-fp32 tests (gradient inputs)
TWO_CASES = ((784, 150, 10), (52, 40, 7))

# The cap rule: err <= factor * max(err of the layered path, 2^-23 * scale), factor 3 (the rough
# geometric midpoint between where the true split lands in the model, <= 0.7 of that cap, and
# where a lost term lands, >= 3.9 x).  FACTORS holds per-(dims, block or "logits") exceptions,
# each 2 x a ratio measured on an MI355X with every term present; test_x6_model_cpu.py keeps
# each at or below half the smallest lost-term ratio of its block and case.
FACTOR = 3.0
FACTORS = {}


def case_id(dims):
    return "x".join(str(v) for v in dims)


def factor(dims, name):
    return FACTORS.get((dims, name), FACTOR)


def module(flat, dims, dtype):
    from distributed_learning_amd.networks import ANNModel
    m = ANNModel(*dims).to(dtype)
    off = 0
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
    return m


def agent(seed, dims, rows=BATCH, data=True):
    """(flat fp32 parameters, data [rows, din], labels int64 [rows]) of one agent."""
    from distributed_learning_amd.networks import ANNModel
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        m = ANNModel(*dims)
        x = torch.randn(rows, dims[0]) if data else None
        y = torch.randint(0, dims[2], (rows,)) if data else None
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]), x, y


def shared_rows(dims):
    gen = torch.Generator().manual_seed(LOGIT_DATA_SEED)
    return torch.randn(LOGIT_ROWS, dims[0], generator=gen)


def relu_margin(flat, x, dims):
    """(m, e): min |z1| of the fp64 forward, and the largest |z1(fp32 on the CPU) - z1(fp64)|."""
    with torch.no_grad():
        z64 = module(flat, dims, torch.float64).fc1(x.double())
        z32 = module(flat, dims, torch.float32).fc1(x)
    return float(z64.abs().min()), float((z32.double() - z64).abs().max())


def search_seeds(dims, n=2, rows=None, limit=200):
    """The first n seeds (0, 1, ...) whose margin is >= SEARCH_RATIO x the fp32 error; rows=None:
    a gradient case (the agent's own batch), else the shared logits rows."""
    found = []
    x_shared = None if rows is None else shared_rows(dims)
    for seed in range(limit):
        flat, x, _ = agent(seed, dims, data=rows is None)
        m, e = relu_margin(flat, x if rows is None else x_shared, dims)
        if m >= SEARCH_RATIO * e:
            found.append(seed)
            if len(found) == n:
                return tuple(found)
    raise RuntimeError(f"no {n} seeds below {limit} for {dims}")


@functools.lru_cache(maxsize=None)
def grad_oracle(dims):
    """The case's inputs and its float64 gradients, loss, logits and margins, computed once:
    dict of X [n, P] fp32, data [n, 64, din], labels int32 [n, 64], G64 [n, P], loss64 [n],
    z64 [n, 64, dout], margins [(m, e)]."""
    flats, xs, ys, grads, losses, zs, margins = [], [], [], [], [], [], []
    for seed in GRAD_CASES[dims]:
        flat, x, y = agent(seed, dims)
        m = module(flat, dims, torch.float64)
        z = m(x.double())
        loss = F.cross_entropy(z, y)
        loss.backward()
        flats.append(flat), xs.append(x), ys.append(y), zs.append(z.detach())
        grads.append(torch.cat([p.grad.reshape(-1) for p in m.parameters()]))
        losses.append(loss.detach())
        margins.append(relu_margin(flat, x, dims))
    return dict(X=torch.stack(flats), data=torch.stack(xs), labels=torch.stack(ys).int(),
                G64=torch.stack(grads), loss64=torch.stack(losses), z64=torch.stack(zs),
                margins=margins)


@functools.lru_cache(maxsize=None)
def logit_oracle(dims):
    """dict of X [n, P] fp32, data [130, din] (shared), z64 [n, 130, dout], margins."""
    x = shared_rows(dims)
    flats = [agent(seed, dims, data=False)[0] for seed in LOGIT_CASES[dims]]
    with torch.no_grad():
        z = torch.stack([module(f, dims, torch.float64)(x.double()) for f in flats])
    return dict(X=torch.stack(flats), data=x, z64=z,
                margins=[relu_margin(f, x, dims) for f in flats])
