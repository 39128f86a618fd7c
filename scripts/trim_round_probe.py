"""The trimmed-mean round (dl_trim_round, with g) against the plain round (dl_mix_round, with g)
at the c2 shape: 1024 agents x 2^20 params, on the committed 4-regular graph and on an 8-regular
circulant, row-major and column-tiled, with and without the deviation.  Both rounds move the same
12 B per element; what differs is the fold (a sorting network against a weighted sum), so the
ratio trim / mix is the cost of the screening.

The four forms (mix, trim, each with the deviation) run interleaved in one process, one HIP-event
pair per round after warm-up.  The samples are taken in --blocks blocks of --rounds each; every
form's median is reported per block and overall, and the spread between a form's block medians is
the yardstick a difference must exceed.

  python scripts/trim_round_probe.py [--agents 1024 --params 1048576 --rounds 20 --blocks 3]

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


def probe(dev, name, csr, n, P, layout, trim, rounds, blocks, warmup):
    eng = engine.GossipEngine(csr, P, device=dev, layout=layout)
    tiled = (P, eng.T) if eng.layout == "tiled" else None
    X, Y = eng.X, eng.Y
    G = eng._empty()
    gen = torch.Generator(device=dev).manual_seed(0)
    X.normal_(generator=gen)
    G.normal_(generator=gen)
    kw = dict(workspace=eng.ws, tiled=tiled)
    dv = dict(dev_sq=eng.dev_sq, dev_max=eng.dev_max)
    plan = engine.trim_round_plan(eng.W, X, Y, G, trim=trim, deviation=True, tiled=tiled)
    if plan is None:
        raise SystemExit("the trimmed-mean round does not take this shape")

    def mix(**dev_kw):
        engine.mix_round(eng.W, X, Y, G=G, lr=LR, **dev_kw, **kw)

    def trimmed(**dev_kw):
        assert engine.trim_round(eng.W, X, Y, G, LR, trim, **dev_kw, **kw)

    cases = [("mix", mix), ("trim", trimmed), ("mix_dev", lambda: mix(**dv)),
             ("trim_dev", lambda: trimmed(**dv))]
    for _ in range(warmup):
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k, _ in cases}
    for _ in range(rounds * blocks):
        for k, fn in cases:          # interleaved: every form sees the same machine state
            ev[k].append(timed(fn))
    torch.cuda.synchronize()
    res = {k: summary([s.elapsed_time(e) for s, e in v], blocks) for k, v in ev.items()}
    tbs = lambda r: round(12 * n * P / (r["median_ms"] / 1e3) / 1e12, 3)  # noqa: E731
    out = {"case": f"{name} {eng.layout}", "agents": n, "params": P, "trim": trim, "plan": plan,
           **res}
    for t, m in (("trim", "mix"), ("trim_dev", "mix_dev")):
        out[t + "_vs_" + m] = {
            "ratio": round(res[t]["median_ms"] / res[m]["median_ms"], 4),
            "spread_ms": max(res[t]["block_spread_ms"], res[m]["block_spread_ms"]),
            "trim_TBs_at_12B": tbs(res[t]), "mix_TBs_at_12B": tbs(res[m])}
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
        raise SystemExit("trim_round_probe measures on the GPU; none is available")
    dev = torch.device("cuda", 0)
    graphs = {"regular4": lambda: (bench.build_graph(args.agents)[0], 1),
              "circulant8": lambda: (circulant(args.agents, 4), 2)}
    for name in [v for v in args.graphs.split(",") if v]:
        csr, trim = graphs[name]()
        for layout in [v for v in args.layouts.split(",") if v]:
            probe(dev, name, csr, args.agents, args.params, layout, trim, args.rounds,
                  args.blocks, args.warmup)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
