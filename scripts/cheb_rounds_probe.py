"""Rounds/s of the multi-round Chebyshev pass (dl_cheb_rounds) against the per-round dl_cheb_round
loop and the plain multi-round pass (dl_mix_rounds, the LDS ceiling), in one process: HIP events,
the forms interleaved, medians of 30 in three blocks of 10 with the spread between the block
medians.  Shapes: c2 (1024 agents x 2^20, 4-regular, 16-column tiles) and c4 (64 x 64 torus, 4096
agents x 2^18, 4-column tiles), column-tiled, 4 GiB of X each (--params-mb).  Then end to end:
mix_chebyshev to eps 1e-3 on the torus with best-constant weights, passes against the per-round
loop.

    python scripts/cheb_rounds_probe.py [--params-mb 4096] > profiles/r30/cheb_rounds/probe.log
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_learning_amd import engine as E, graph as G   # noqa: E402


def timed(fn, rounds, blocks=3, per=10):
    fn()
    torch.cuda.synchronize()
    meds = []
    for _ in range(blocks):
        ts = []
        for _ in range(per):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        meds.append(float(np.median(ts)))
    med = float(np.median(meds))
    return {"rounds_per_s": rounds / med, "ms": med * 1e3,
            "spread_pct": 100.0 * (max(meds) - min(meds)) / med}


def regular_graph(n, seed):
    edges = G.random_regular_edges(4, n, seed=seed)
    return G.from_edge_weights(edges, [0.2] * len(edges), list(range(n)))


def torus_graph():
    e = G.torus_edges(64, 64)
    w = 2.0 / (2.0 - 2.0 * math.cos(2 * math.pi / 64) + 8.0)
    return G.from_edge_weights(e, [w] * len(e), list(range(4096)))


def probe(name, csr, T, mb, dev):
    n = csr.n_rows
    P = max(T, (mb << 20) // (4 * n) // T * T)
    W = E.DeviceCsr(csr, dev)
    tiled = (P, T)
    mk = lambda: torch.randn(E.tiled_shape(n, P, T), device=dev)   # noqa: E731
    X, Y, Z, Zo = mk(), mk(), mk(), mk()
    coef = torch.tensor([1.3, -0.3] * 64, device=dev)
    trace = torch.zeros(E.CHEB_TRACE_ROUNDS, device=dev)
    ws = E.Workspace(dev)
    forms = {}
    for K in (16, 64):
        forms[f"cheb_rounds K={K}"] = (K, lambda K=K: E.cheb_rounds(W, X, Y, Z, Zo, coef, K,
                                                                      workspace=ws, tiled=tiled))
        forms[f"mix_rounds K={K}"] = (K, lambda K=K: E.mix_rounds(W, X, Y, K, workspace=ws,
                                                                   tiled=tiled))
    KT = E.CHEB_TRACE_ROUNDS
    forms[f"cheb_rounds traced K={KT}"] = (KT, lambda: E.cheb_rounds(W, X, Y, Z, Zo, coef, KT,
                                                                      trace=trace, workspace=ws,
                                                                      tiled=tiled))
    forms["cheb_round loop (8 launches)"] = (8, lambda: [E.cheb_round(W, X, Z, Z, 1.3, -0.3,
                                                                       workspace=ws, tiled=tiled)
                                                         for _ in range(8)])
    for label, (K, fn) in forms.items():
        assert fn() is not False, label
        r = timed(fn, K)
        print(json.dumps({"shape": name, "n": n, "P": P, "T": T, "form": label, **r}), flush=True)


def end_to_end(dev):
    csr = torus_graph()
    n, P = 4096, 4096
    Wd = np.zeros((n, n))
    for a in range(n):
        Wd[a, csr.col[csr.rowptr[a]:csr.rowptr[a + 1]]] = csr.w[csr.rowptr[a]:csr.rowptr[a + 1]]
    gamma = float(np.abs(np.linalg.eigvalsh(Wd - 1.0 / n)).max())
    X0 = torch.randn(n, P, device=dev)
    for passes in (False, True):
        def run():
            eng = E.GossipEngine(csr, P, device=dev, X=X0, layout="tiled", tile_cols=4)
            run.done = eng.mix_chebyshev(gamma, 1, 1e-3, passes=passes)
        r = timed(run, 1)
        print(json.dumps({"shape": "torus 4096 x 4096 to eps 1e-3 (engine set-up included)",
                          "passes": passes, "rounds": run.done, "ms": r["ms"],
                          "spread_pct": r["spread_pct"]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--params-mb", type=int, default=4096)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    probe("c2", regular_graph(1024, 1), 16, a.params_mb, dev)
    probe("c4", torus_graph(), 4, a.params_mb, dev)
    end_to_end(dev)
