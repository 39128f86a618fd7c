"""CPU checks of dl_drop_rounds' contract: the link hash restated in numpy (known answers, the
library's dl_link_mask against it, symmetry, the down fraction) and every refusal of the pass with
its status and text, before any device call."""
import ctypes

import numpy as np
import pytest


def fmix(a):
    a = np.array(a, np.uint32, ndmin=1)
    a ^= a >> 16
    a *= np.uint32(0x85EBCA6B)
    a ^= a >> 13
    a *= np.uint32(0xC2B2AE35)
    a ^= a >> 16
    return a


def u(seed, t, lo, hi):
    key = fmix((seed + 0x9E3779B9 * (t + 1)) % 2 ** 32)
    return fmix(fmix(key ^ np.asarray(lo, np.uint32)) ^ np.asarray(hi, np.uint32))


def thr(p):
    return min(int(p * 2 ** 32), 2 ** 32 - 1)


def up_mask(csr, seed, t, p_edge, p_node):
    """Per CSR entry: is it up in round t (a row's first entry and diagonal entries always)."""
    rp, col = np.asarray(csr.rowptr), np.asarray(csr.col)
    row = np.repeat(np.arange(csr.n_rows), np.diff(rp))
    down = (u(seed, t, np.minimum(row, col), np.maximum(row, col)) < thr(p_edge)) | \
           (u(seed, t, row, row) < thr(p_node)) | (u(seed, t, col, col) < thr(p_node))
    down[row == col] = False
    down[rp[:-1]] = False
    return ~down


def test_known_answers():
    assert u(0, 0, 0, 1)[0] == 0xfb49e243 and u(5, 9, 3, 3)[0] == 0x127b72b0


@pytest.mark.parametrize("seed,t", [(0, 0), (7, 3), (12345, 2 ** 32 - 1)])
def test_link_mask_is_the_restatement_and_symmetric(seed, t):
    from distributed_learning_amd import graph as G
    csr = G.barabasi_albert_metropolis(100, 2, seed=5)
    got = G.link_mask(csr, seed, t, 0.3, 0.2)
    assert got.dtype == np.uint8 and np.array_equal(got, up_mask(csr, seed, t, 0.3, 0.2))
    assert 0 < got.sum() < got.size
    row = np.repeat(np.arange(csr.n_rows), np.diff(csr.rowptr))
    state = {(int(i), int(j)): int(b) for i, j, b in zip(row, csr.col, got)}
    assert all(state[(j, i)] == b for (i, j), b in state.items())


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_down_fraction(seed):
    """2048 links (a ring) x 32 rounds at p = 0.3: within 5 sigma, sigma = sqrt(0.21 / 65536)."""
    from distributed_learning_amd import graph as G
    n = 2048
    csr = G.from_edge_weights([(i, (i + 1) % n) for i in range(n)], [0.25] * n, list(range(n)))
    row = np.repeat(np.arange(n), np.diff(csr.rowptr))
    once = row < np.asarray(csr.col)   # each link's entry in its lower end's row
    assert once.sum() == n
    down = sum(int((G.link_mask(csr, seed, t, 0.3)[once] == 0).sum()) for t in range(32))
    assert abs(down / 65536 - 0.3) <= 5 * np.sqrt(0.21 / 65536)


def ring_args(n=64, P=256, tile_cols=0):
    """dl_drop_rounds_args of a shared-weight ring with made-up (never read) device addresses."""
    from distributed_learning_amd import _lib
    a = _lib.DlDropRoundsArgs()
    m = a.mix
    m.x, m.y, m.n_params, m.tile_cols = 1 << 30, 1 << 32, P, tile_cols
    m.ldx = m.ldy = 0 if tile_cols else P
    m.W = _lib.DlCsr(1 << 20, 1 << 21, 1 << 22, n, 3 * n, 3, 1, 1)
    a.rounds, a.thr_edge = 4, thr(0.3)
    return a


REFUSALS = [   # (what to set, status name, text)
    (lambda a: setattr(a, "rounds", 0), "DL_ERR_INVALID", b"rounds must be >= 1"),
    (lambda a: setattr(a.mix, "mean_prev", 4096), "DL_ERR_UNSUPPORTED", b"no halo rows"),
    (lambda a: setattr(a.mix, "n_local_src", 32), "DL_ERR_UNSUPPORTED", b"partition row sets"),
    ("gather", "DL_ERR_UNSUPPORTED", b"plan path 1"),
    (lambda a: setattr(a.mix, "x", (1 << 30) + 4), "DL_ERR_UNSUPPORTED", b"16-byte aligned"),
    ("wide", "DL_ERR_UNSUPPORTED", b"do not fit LDS"),
    (lambda a: (setattr(a.mix, "dev_sq", 1 << 34), setattr(a.mix.W, "doubly_stochastic", 0)),
     "DL_ERR_UNSUPPORTED", b"doubly stochastic"),
]


@pytest.mark.parametrize("change,status,text", REFUSALS, ids=[r[2].decode() for r in REFUSALS])
def test_refusals_before_any_device_call(monkeypatch, change, status, text):
    from distributed_learning_amd import _lib
    lib, plan = _lib.load(), _lib.DlMixPlan()
    good = ring_args()
    assert lib.dl_drop_rounds_plan(ctypes.byref(good), ctypes.byref(plan)) == _lib.DL_OK
    assert plan.path == 3 and plan.tile_cols >= 4
    a = ring_args()
    if change == "gather":
        monkeypatch.setenv("DLAMD_FORCE_GATHER", "1")
    elif change == "wide":   # one 16-column image of 1300 rows fits LDS, two do not
        a = ring_args(n=1300, tile_cols=16)
    else:
        change(a)
    if text != b"16-byte aligned":   # (the plan query does not look at the addresses)
        assert lib.dl_drop_rounds_plan(ctypes.byref(a), ctypes.byref(plan)) == getattr(_lib, status)
        assert text in lib.dl_last_error(), lib.dl_last_error()
    # the pass itself: shaped on the host, refused before anything is launched
    assert lib.dl_drop_rounds(ctypes.byref(a), None, 0, None) == getattr(_lib, status)
    assert text in lib.dl_last_error(), lib.dl_last_error()
