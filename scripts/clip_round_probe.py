"""Clipped gossip (GossipEngine.round_clip) and its distance pass (dl_edge_sqdist) against the
plain round (dl_mix_round, with g) at the c2 shape: 1024 agents x 2^20 params, on the committed
4-regular graph and on an 8-regular circulant, row-major and column-tiled.  The distance pass
moves 8 B per element with g and 4 B without, the plain round 12 B, the whole round_clip 20 B
(the pass, a one-thread-per-row launch, then dl_mix_round with per-edge weights).

The five forms -- the pass without and with g, round_clip, dl_mix_round with g on W and on the
clipped weights Wc (per-edge, not shared between rows) -- run interleaved in one process, one
HIP-event pair per call after warm-up.  The samples are taken in --blocks blocks of --rounds
each; every form's median is reported per block and overall, and the spread between a form's
block medians is the yardstick a difference must exceed.

  python scripts/clip_round_probe.py [--agents 1024 --params 1048576 --rounds 20 --blocks 3]

One JSON line per graph and layout."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from distributed_learning_amd import engine  # noqa: E402
from distributed_learning_amd.graph import Csr  # noqa: E402
import bench  # noqa: E402

LR = 0.05


def circulant(n, half):
    """Every agent and its +-1 ... +-half neighbours, uniform weights."""
    cols = np.concatenate([[a] + [(a + d) % n for d in range(1, half + 1)] +
                           [(a - d) % n for d in range(1, half + 1)] for a in range(n)])
    k = 2 * half + 1
    return Csr(np.arange(0, k * n + 1, k), cols, np.full(cols.size, 1.0 / k))


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    return s, e


def summary(ms, blocks):
    per = len(ms) // blocks
    meds = [statistics.median(ms[b * per:(b + 1) * per]) for b in range(blocks)]
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "block_medians_ms": [round(m, 4) for m in meds],
            "block_spread_ms": round(max(meds) - min(meds), 4), "samples": len(ms)}


def probe(dev, name, csr, n, P, layout, rounds, blocks, warmup):
    eng = engine.GossipEngine(csr, P, device=dev, layout=layout)
    tiled = (P, eng.T) if eng.layout == "tiled" else None
    G = eng._empty()
    gen = torch.Generator(device=dev).manual_seed(0)
    eng.X.normal_(generator=gen)
    G.normal_(generator=gen)
    eng.reserve_workspace(deviation=True, clip=True)
    kw = dict(workspace=eng.ws, tiled=tiled)
    plan = engine.edge_sqdist_plan(eng.W, eng.X, G, tiled=tiled)
    if plan is None:
        raise SystemExit("the distance pass does not take this shape")

    def edge(g=None):
        assert engine.edge_sqdist(eng.W, eng.X, g, LR, out=eng.edge_sq, **kw) is not False

    def mix(W):
        engine.mix_round(W, eng.X, eng.Y, G=G, lr=LR, **kw)

    # (round_clip swaps X and Y; the operands of every other form are looked up per call)
    cases = [("edge", edge), ("edge_g", lambda: edge(G)),
             ("round_clip", lambda: eng.round_clip(G, LR, drop=1)),
             ("mix", lambda: mix(eng.W)), ("mix_edge_weights", lambda: mix(eng.Wc))]
    for _ in range(warmup):
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k, _ in cases}
    for _ in range(rounds * blocks):
        eng.X.normal_(generator=gen)     # (the clipped rounds contract X towards consensus)
        for k, fn in cases:          # interleaved: every form sees the same machine state
            ev[k].append(timed(fn))
    torch.cuda.synchronize()
    res = {k: summary([s.elapsed_time(e) for s, e in v], blocks) for k, v in ev.items()}
    byt = {"edge": 4, "edge_g": 8, "round_clip": 20, "mix": 12, "mix_edge_weights": 12}
    for k, r in res.items():
        r["TBs"] = round(byt[k] * n * P / (r["median_ms"] / 1e3) / 1e12, 3)
    out = {"case": f"{name} {eng.layout}", "agents": n, "params": P, "plan": plan, **res}
    for t in ("edge", "edge_g", "round_clip", "mix_edge_weights"):
        out[t + "_vs_mix"] = {
            "ratio": round(res[t]["median_ms"] / res["mix"]["median_ms"], 4),
            "spread_ms": max(res[t]["block_spread_ms"], res["mix"]["block_spread_ms"])}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--params", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layouts", default="rows,tiled")
    ap.add_argument("--graphs", default="regular4,circulant8")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_round_probe measures on the GPU; none is available")
    dev = torch.device("cuda", 0)
    graphs = {"regular4": lambda: bench.build_graph(args.agents)[0],
              "circulant8": lambda: circulant(args.agents, 4)}
    for name in [v for v in args.graphs.split(",") if v]:
        csr = graphs[name]()
        for layout in [v for v in args.layouts.split(",") if v]:
            probe(dev, name, csr, args.agents, args.params, layout, args.rounds,
                  args.blocks, args.warmup)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
