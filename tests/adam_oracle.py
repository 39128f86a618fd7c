"""numpy restatement of the Adam step and round (dl_adam_step, dl_adam_round, dl_adam_tick;
include/dlamd.h), shared by test_adam_host.py and test_adam_round_gpu.py: every line of the
definition is one fp32 numpy operation (numpy rounds each to nearest and its float32 sqrt and
divide are the correctly rounded ones), the step count's recurrence runs in Python floats, and
the round is that step followed by the oracle's fold (cref.mix_round, bit for bit
Mixer._mix_params_once)."""
import math

import numpy as np

from oracle import cref

f32 = np.float32


class Coefs:
    """The recurrence of dl_adam_tick: t, beta1^t and beta2^t by one multiply a step from 1.0,
    step_size = fl32(lr / (1 - beta1^t)) and bias2_sqrt = fl32(sqrt(1 - beta2^t)) in fp64."""

    def __init__(self, lr, betas=(0.9, 0.999)):
        self.lr, self.beta1, self.beta2 = float(lr), float(betas[0]), float(betas[1])
        self.t, self.b1t, self.b2t = 0, 1.0, 1.0

    def tick(self):
        self.t += 1
        self.b1t *= self.beta1
        self.b2t *= self.beta2
        return self

    @property
    def step_size(self):
        return f32(self.lr / (1.0 - self.b1t))

    @property
    def bias2_sqrt(self):
        return f32(math.sqrt(1.0 - self.b2t))

    def state(self):
        """The float64[8] device state after these ticks, the coefficient slot as two floats."""
        s = np.array([self.t, self.b1t, self.b2t, self.lr, self.beta1, self.beta2, 0.0, 0.0])
        if self.t > 0:      # (zero until the first tick)
            s[6:7].view(np.float32)[:] = [self.step_size, self.bias2_sqrt]
        return s


def adam_step(X, G, M, V, lr, step_size, bias2_sqrt, betas=(0.9, 0.999), eps=1e-8,
              weight_decay=0.0, decoupled=False):
    """(S, M', V') of one step; nothing is modified.  step_size, bias2_sqrt: ``Coefs``."""
    x, g, m, v = (np.asarray(a, f32) for a in (X, G, M, V))
    omb1 = f32(1.0 - float(betas[0]))
    omb2 = f32(1.0 - float(betas[1]))
    b2 = f32(betas[1])
    ss, bs, e = f32(step_size), f32(bias2_sqrt), f32(eps)
    with np.errstate(all="ignore"):
        if weight_decay != 0.0:
            if decoupled:
                x = x * f32(1.0 - float(f32(lr)) * float(f32(weight_decay)))
            else:
                g = f32(weight_decay) * x + g
        m = m + omb1 * (g - m)
        v = b2 * v + (omb2 * g) * g
        den = np.sqrt(v) / bs + e
        s = x - ss * (m / den)
    assert s.dtype == m.dtype == v.dtype == np.float32
    return s, m, v


def adam_round(csr, X, G, M, V, lr, step_size, bias2_sqrt, **opt):
    """(X', M', V') of one round: the step, then the mix of the stepped rows."""
    S, M, V = adam_step(X, G, M, V, lr, step_size, bias2_sqrt, **opt)
    with np.errstate(all="ignore"):
        return cref.mix_round(S, csr.rowptr, csr.col, csr.w), M, V


def adam_rounds(csr, X, Gs, lr, M=None, V=None, **opt):
    """[(X, M, V) after round 1, 2, ...] from m = v = 0 (or M, V) at t = 0."""
    M = np.zeros_like(X) if M is None else M
    V = np.zeros_like(X) if V is None else V
    c = Coefs(lr, opt.get("betas", (0.9, 0.999)))
    out = []
    for G in Gs:
        c.tick()
        X, M, V = adam_round(csr, X, G, M, V, lr, c.step_size, c.bias2_sqrt, **opt)
        out.append((X, M, V))
    return out
