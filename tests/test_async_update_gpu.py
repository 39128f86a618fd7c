"""``dl_async_load`` / ``dl_async_update`` / ``dl_async_read`` (csrc/async_mix.hip) against numpy
itself (tests/jacobi_oracle.async_load / async_update: the reference's expressions,
consensus_asyncio.py:231, :295, :297), bit for bit -- through ``DeviceIterates`` where the class
can express the case, through the C ABI where it cannot (a chosen arena stride, the parity of the
flag words, the argument refusals).  Reached here and nowhere else in the suite:

* ``pairwise_sum`` at d = 8 exactly, in its 8-wide loop body (d >= 16) and its tails, fp64 and
  ``sum_f32``; d = 0;
* more than one workgroup: the cross-workgroup atomicOr into ``flags[parity]``, the 1024-block
  grid cap and the grid-stride loop behind it (262147 = 1024 * 256 + 3 elements);
* ``ld > n_params``; both parities; every argument refusal, none of which launches anything."""
import ctypes

import numpy as np
import pytest
import torch

import jacobi_cases as C
import jacobi_oracle as O

pytestmark = pytest.mark.gpu

FILL = -3.0517578125e-05       # what unused arena elements hold before and after
CAP = 1024 * 256               # elements the capped grid covers in one pass
N_BIG = CAP + 3


def _lib():
    from distributed_learning_amd import _lib
    return _lib


class Arena:
    """A caller-owned arena [slots, ld] with values V in its first rows and columns."""

    def __init__(self, cuda, V, n_slots, ld, flags=(0, 0)):
        self.cuda, self.ld, self.n = cuda, ld, V.shape[1]
        self.host = np.full((n_slots, ld), FILL)
        self.host[:V.shape[0], :self.n] = V
        self.dev = torch.from_numpy(self.host).to(cuda)
        self.flags = torch.tensor(flags, dtype=torch.int32, device=cuda)

    def update(self, self_slot, out_slot, nbrs, sum_f32, keep, eps, conv, parity, n=None,
               ld=None, n_nbrs=None):
        L = _lib()
        a = L.DlAsyncUpdateArgs()
        a.arena, a.ld = self.dev.data_ptr(), self.ld if ld is None else ld
        a.n_params = self.n if n is None else n
        a.self_slot, a.out_slot = self_slot, out_slot
        a.n_nbrs = len(nbrs) if n_nbrs is None else n_nbrs
        for j, s in enumerate(nbrs):
            a.nbr_slots[j] = s
        a.sum_f32, a.keep, a.eps, a.conv_eps = sum_f32, keep, eps, conv
        a.flags, a.parity = self.flags.data_ptr(), parity
        verdict = ctypes.c_int32(-1)
        rc = L.load().dl_async_update(ctypes.byref(a), ctypes.byref(verdict),
                                      L.stream_handle(self.cuda))
        return rc, verdict.value

    def read(self):
        torch.cuda.synchronize()
        return self.dev.cpu().numpy(), self.flags.cpu().tolist()


def _keep_eps(d):
    eps = 0.95 / max(d, 1)
    return float(np.float64(1) - np.float64(eps) * d), eps


@pytest.mark.parametrize("f32", [0, 1])
def test_scalar_values_pairwise_sum(cuda, f32):
    """n_params == 1 through DeviceIterates: a stack of d scalars sums pairwise, in fp64 or (all
    neighbours fp32 pre-scaled values) in fp32; the verdict at a conv_eps far on either side."""
    from distributed_learning_amd.iterates import DeviceIterates
    it = DeviceIterates(cuda)
    for d in C.ASYNC_D:
        v = C.async_scalars(d, f32)
        # weight = mean_weight = 1: the pre-scale is the identity, its dtype decides sum_f32
        h = [it.load(np.float32(x) if f32 else float(x), 1, 1) for x in v]
        assert all(y.f32 == bool(f32) for y in h)
        keep, eps = _keep_eps(d)
        for conv, verdict in ((1e30, True), (-1e30, d == 0)):
            want, ok = O.async_update(np.float64(v[0]), [np.float64(x) for x in v[1:]], keep,
                                      eps, conv, bool(f32) and d > 0)
            got, flag = it.update(h[0], h[1:], keep, eps, conv)
            assert ok == verdict == flag, (d, conv)
            assert O.same_bits(np.float64(got.value()), np.float64(want)), (d, got.value(), want)


@pytest.mark.parametrize("f32", [0, 1])
def test_scalar_values_abi(cuda, f32):
    """The same sums through the ABI with ld = 3 > n_params = 1, sum_f32 also at d = 0."""
    for d in C.ASYNC_D:
        v = C.async_scalars(d, f32)
        ar = Arena(cuda, v[:, None], d + 2, 3)
        keep, eps = _keep_eps(d)
        want, ok = O.async_update(np.float64(v[0]), [np.float64(x) for x in v[1:]], keep, eps,
                                  1e30, bool(f32))
        rc, verdict = ar.update(0, d + 1, list(range(1, d + 1)), f32, keep, eps, 1e30, d & 1)
        assert rc == 0 and verdict == 1 == int(ok)
        exp = ar.host.copy()
        exp[d + 1, 0] = want
        got, flags = ar.read()
        assert O.same_bits(got, exp), (d, got[d + 1, 0], want)
        assert flags == [0, 0]


@pytest.mark.parametrize("n", [2, 255, 256, 257, N_BIG])
def test_vector_values(cuda, n):
    """One workgroup, the workgroup boundary, and one element past the grid cap; d = 1 and 4,
    fp64 and fp32 sums, an arena wider than the values.  Everything but the output slot's first
    n elements keeps its bits."""
    for d in (1, 4):
        for f32 in (0, 1):
            V = C.async_vectors(n, d, f32)
            ar = Arena(cuda, V, d + 2, n + 5)
            keep, eps = _keep_eps(d)
            want, ok = O.async_update(V[0], list(V[1:]), keep, eps, 1e30, bool(f32))
            rc, verdict = ar.update(0, d + 1, list(range(1, d + 1)), f32, keep, eps, 1e30, 1)
            assert rc == 0 and verdict == 1 == int(ok)
            exp = ar.host.copy()
            exp[d + 1, :n] = want
            got, flags = ar.read()
            assert O.same_bits(got, exp), (d, f32, int((got != exp).sum()))
            assert flags == [0, 0]


def test_vector_values_through_device_iterates(cuda):
    from distributed_learning_amd.iterates import DeviceIterates
    it = DeviceIterates(cuda)
    for f32 in (0, 1):
        V = C.async_vectors(257, 4, f32)
        h = [it.load(x.astype(np.float32) if f32 else x, 1, 1) for x in V]
        keep, eps = _keep_eps(4)
        want, ok = O.async_update(V[0], list(V[1:]), keep, eps, 1e30, bool(f32))
        got, flag = it.update(h[0], h[1:], keep, eps, 1e30)
        assert flag and ok and O.same_bits(got.value(), want)


@pytest.mark.parametrize("where,p", [("first workgroup", 5), ("last workgroup", 1023 * 256 + 7),
                                     ("grid-stride tail", CAP + 2)])
def test_verdict_crosses_workgroups(cuda, where, p):
    """Every agent holds the same vector, so y' - v is rounding noise against conv_eps = 1e-3;
    one neighbour is 1.0 lower in ONE element, which then fails by about 0.7.  That element's
    workgroup alone must turn the verdict, wherever it runs; the next call (other parity, the
    element repaired) converges, and each call leaves the other parity's flag word zero."""
    d, n = 3, N_BIG
    x = np.random.default_rng(3).standard_normal(n)
    V = np.stack([x] * (d + 1))
    V[2, p] -= 1.0
    ar = Arena(cuda, V, d + 3, n + 1, flags=(0, 1))
    keep, eps = _keep_eps(d)
    want, ok = O.async_update(V[0], list(V[1:]), keep, eps, 1e-3, False)
    gaps = np.stack([want - v for v in V[1:]])
    assert not ok and (gaps > 1e-3).sum() == 1 and gaps[1, p] > 0.5
    assert np.delete(gaps.reshape(-1), n + p).max() < 1e-9      # the rest: 1e6 below conv_eps
    rc, verdict = ar.update(0, d + 1, [1, 2, 3], 0, keep, eps, 1e-3, 0)
    assert rc == 0 and verdict == 0
    got, flags = ar.read()
    assert flags == [1, 0] and O.same_bits(got[d + 1, :n], want)
    # second call: the repaired neighbour sits in slot d + 2
    fixed = torch.from_numpy(x).to(cuda)
    ar.dev[d + 2, :n] = fixed
    want2, ok2 = O.async_update(V[0], [V[1], x, V[3]], keep, eps, 1e-3, False)
    assert ok2
    rc, verdict = ar.update(0, d + 1, [1, d + 2, 3], 0, keep, eps, 1e-3, 1)
    assert rc == 0 and verdict == 1
    got, flags = ar.read()
    assert flags == [0, 0] and O.same_bits(got[d + 1, :n], want2)


@pytest.mark.parametrize("n", [1, 257, N_BIG])
@pytest.mark.parametrize("mode", [0, 1])
def test_load_and_read(cuda, n, mode):
    """v * w / m in fp64 (mode 0) or fp32 (mode 1, weights pre-rounded to fp32 as iterates.py
    passes them), into a slot of a wider arena; dl_async_read returns the slot's bits."""
    L = _lib()
    lib = L.load()
    v = C.async_vectors(n, 0, mode)[0]
    w, m = (float(np.float32(3.3)), float(np.float32(4.7))) if mode else (3.3, 4.7)
    ar = Arena(cuda, np.zeros((0, n)), 3, n + 3)
    a = L.DlAsyncLoadArgs()
    a.arena, a.ld, a.n_params, a.slot, a.mode = ar.dev.data_ptr(), ar.ld, n, 1, mode
    a.src, a.weight, a.mean_weight = v.ctypes.data, w, m
    assert lib.dl_async_load(ctypes.byref(a), L.stream_handle(cuda)) == 0
    want = O.async_load(v, w, m, mode)
    assert want.dtype == np.float64 and np.array_equal(want, v * w / m) == (mode == 0)
    exp = ar.host.copy()
    exp[1, :n] = want
    got, _ = ar.read()
    assert O.same_bits(got, exp)
    back = np.full(n + 2, FILL)
    assert lib.dl_async_read(ar.dev.data_ptr(), ar.ld, 1, n, back.ctypes.data,
                             L.stream_handle(cuda)) == 0
    assert O.same_bits(back[:n], want) and O.same_bits(back[n:], np.full(2, FILL))


def test_refusals_launch_nothing(cuda):
    L = _lib()
    V = C.async_vectors(7, 3, 0)
    ar = Arena(cuda, V, 6, 9, flags=(3, 5))
    ok = dict(self_slot=0, out_slot=4, nbrs=[1, 2, 3], sum_f32=0, keep=0.05, eps=0.3, conv=1.0,
              parity=0)
    bad = [(dict(nbrs=[1] * 64, n_nbrs=65), L.DL_ERR_UNSUPPORTED),
           (dict(out_slot=0), L.DL_ERR_INVALID),
           (dict(nbrs=[1, 4, 3]), L.DL_ERR_INVALID),
           (dict(ld=6), L.DL_ERR_INVALID),
           (dict(parity=2), L.DL_ERR_INVALID),
           (dict(n=0), L.DL_ERR_INVALID),
           (dict(nbrs=[], n_nbrs=-1), L.DL_ERR_INVALID)]
    for change, status in bad:
        rc, verdict = ar.update(**{**ok, **change})
        assert rc == status and verdict == -1, change
        got, flags = ar.read()
        assert O.same_bits(got, ar.host) and flags == [3, 5], change
    lib = L.load()
    a = L.DlAsyncLoadArgs()
    src = np.ones(7)
    a.arena, a.ld, a.n_params, a.slot, a.src = ar.dev.data_ptr(), 9, 7, 5, src.ctypes.data
    a.weight = a.mean_weight = 1.0
    for field, value in (("mode", 2), ("ld", 6), ("slot", -1), ("n_params", 0)):
        keep = getattr(a, field)
        setattr(a, field, value)
        assert lib.dl_async_load(ctypes.byref(a), L.stream_handle(cuda)) == L.DL_ERR_INVALID
        setattr(a, field, keep)
    out = np.zeros(7)
    assert lib.dl_async_read(ar.dev.data_ptr(), 6, 0, 7, out.ctypes.data,
                             L.stream_handle(cuda)) == L.DL_ERR_INVALID
    got, flags = ar.read()
    assert O.same_bits(got, ar.host) and flags == [3, 5] and not out.any()
