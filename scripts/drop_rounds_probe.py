"""Rounds/s of the failing-link pass (dl_drop_rounds) at K = 64 against dl_mix_rounds on the same
operands (the cost of the mask) and 64 dl_mix_round launches (the per-round loop a user of
time-varying graphs has today, not counting its host work), in one process: HIP events, the forms
interleaved block by block, medians of 30 in three blocks of 10 with the spread between the block
medians.  Shapes: c2 (1024 agents x 2^20, 4-regular, 16-column tiles) and c4 (64 x 64 torus, 4096
agents x 2^18, 4-column tiles), column-tiled, 4 GiB of X each (--params-mb).

    python scripts/drop_rounds_probe.py [--params-mb 4096] > profiles/r31/drop_rounds/probe.log
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

K = 64


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def timed(forms, blocks=3, per=10):
    """Every form in every block, so a drift of the box falls on all of them alike."""
    for fn in forms.values():
        assert fn() is not False
    torch.cuda.synchronize()
    meds = {label: [] for label in forms}
    for _ in range(blocks):
        for label, fn in forms.items():
            meds[label].append(float(np.median([one(fn) for _ in range(per)])))
    out = {}
    for label, m in meds.items():
        med = float(np.median(m))
        out[label] = {"rounds_per_s": K / med, "ms": med * 1e3,
                      "spread_pct": 100.0 * (max(m) - min(m)) / med}
    return out


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
    X, Y = (torch.randn(E.tiled_shape(n, P, T), device=dev) for _ in range(2))
    ws = E.Workspace(dev)
    forms = {f"drop_rounds p_edge={p}": (lambda p=p: E.drop_rounds(W, X, Y, K, p, seed=1,
                                                                   workspace=ws, tiled=tiled))
             for p in (0.0, 0.3)}
    forms["drop_rounds p_edge=0.3 p_node=0.1"] = lambda: E.drop_rounds(
        W, X, Y, K, 0.3, 0.1, seed=1, workspace=ws, tiled=tiled)
    forms["mix_rounds"] = lambda: E.mix_rounds(W, X, Y, K, workspace=ws, tiled=tiled)
    forms["mix_round loop (64 launches)"] = lambda: [E.mix_round(W, X, Y, workspace=ws, tiled=tiled)
                                                     for _ in range(K)]
    for label, r in timed(forms).items():
        print(json.dumps({"shape": name, "n": n, "P": P, "T": T, "K": K, "form": label, **r}),
              flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--params-mb", type=int, default=4096)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    probe("c2", regular_graph(1024, 1), 16, a.params_mb, dev)
    probe("c4", torus_graph(), 4, a.params_mb, dev)
