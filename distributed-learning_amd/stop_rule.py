"""The ``max deviation < eps`` half of the reference's stop rule (utils/consensus_simple/
mixer.py:40-41), decided in one place for every route that tests it: the Mixer's resident,
traced and round-loop routes, ``GossipEngine.mix_chebyshev`` and ``HaloShard.mix``.

The reference compares ``max(devs) < eps`` and loops while that is false.  With a NaN parameter
(or an ``inf - inf`` against the column mean) the maximum is NaN, ``nan < eps`` is false for
every eps, and the reference never returns.  No caller can depend on that, so here a NaN
deviation tested against eps raises ``FloatingPointError`` naming the round; an infinite one is
a number like any other: not below eps.  Host code only (numpy), no device work.
"""
import numpy as np

__all__ = ["below_eps", "nan_max", "nan_max_bits_"]


def below_eps(max_dev, eps, round_no):
    """``eps is None or max_dev < eps`` -- the comparison in the operands' own types, as the
    callers had it (an np.float32 deviation against a Python float or an np.float32 eps compares
    in float32, numpy >= 2) -- except that a NaN ``max_dev`` with eps set raises
    ``FloatingPointError``.  ``round_no``: rounds done when the deviation was taken (0 = the
    iterate the call started from), for the message.  With ``eps=None`` nothing is tested and
    ``max_dev`` may be anything, None included."""
    if eps is None:
        return True
    if max_dev != max_dev:
        raise FloatingPointError(
            f"max deviation is NaN after round {int(round_no)}: the parameters hold a NaN, or "
            f"infinities that cancel against the column mean, and no further round can bring it "
            f"below eps={eps}")
    return bool(max_dev < eps)


def nan_max(values):
    """Maximum of a non-empty sequence of deviations that keeps a NaN wherever it stands
    (Python's ``max`` keeps one only in first place), with the type of the element returned."""
    values = list(values)
    for v in values:
        if v != v:
            return v
    return max(values)


def nan_max_bits_(t):
    """Prepare a tensor of non-negative float32 maxima for an integer MAX all-reduce that keeps
    NaN: returns an int32 view of ``t`` (sign bits cleared in place) whose integer order is the
    float order with every NaN above +inf.  Backends' float MAX drops or keeps a NaN depending
    on the operand order; the integer one cannot.  The caller reduces the view; ``t`` then holds
    the result."""
    import torch
    if t.dtype != torch.float32:
        raise ValueError(f"nan_max_bits_ needs float32 (got {t.dtype})")
    t.abs_()
    return t.view(torch.int32)
