"""The dense round (dl_dense_round, with g) against the plain round (dl_mix_round, with g) on the
Csr of the same complete graph K_N with uniform weights, at N = 64 / 128 / 256 agents x 2^20
params, column-tiled and row-major.  Both move 12 B per element; the dense round spends 2 N flops
per element on the matrix cores where the sparse one folds N LDS reads (or, at N = 256, whose
65 536 entries the LDS kernel cannot stage, gathers them through L2: plan path 2).

The two forms run interleaved in one process, one HIP-event pair per round after warm-up.  The
samples are taken in --blocks blocks of --rounds each; every form's median is reported per block
and overall, and the spread between a form's block medians is the yardstick a difference must
exceed.  Every (N, layout) case runs in a child process of its own under --limit seconds, and the
first case that fails or runs out of time ends the probe.

  python scripts/dense_round_probe.py [--agents 64,128,256 --params 1048576 --rounds 20 --blocks 3]

One JSON line per case."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from distributed_learning_amd import engine  # noqa: E402
from distributed_learning_amd.graph import Csr  # noqa: E402

LR = 0.05


def complete(n):
    """K_n with self loops, every weight 1 / n."""
    return Csr(np.arange(0, n * n + 1, n), np.tile(np.arange(n), n), np.full(n * n, 1.0 / n))


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


def probe(dev, n, P, layout, rounds, blocks, warmup):
    W = engine.DeviceCsr(complete(n), dev)
    Wd = torch.full((n, n), 1.0 / n, device=dev)
    T = 0 if layout == "rows" else (64 if n > 128 else 128)
    tiled = (P, T) if T else None
    shape = engine.tiled_shape(n, P, T) if T else (n, P)
    gen = torch.Generator(device=dev).manual_seed(0)
    X, G = (torch.randn(shape, device=dev, generator=gen) for _ in range(2))
    Y = torch.empty_like(X)
    plan = engine.dense_round_plan(Wd, X, Y, G, tiled=tiled)
    # the sparse round where the planner serves this layout (a column-tiled round needs a tile path)
    try:
        mix_plan = engine.plan_shape(W, P, deviation=False, tile_cols=T)
        mix_ok = not T or (mix_plan["path"] in (1, 4, 5) and mix_plan["tile_cols"] == T)
    except ValueError:   # no tile of all rows beside this CSR: the sparse round has no tiled form
        mix_plan, mix_ok = None, False
    ws = engine.Workspace(dev)
    cases = [("dense", lambda: engine.dense_round(Wd, X, Y, G, LR, tiled=tiled))]
    if mix_ok:
        cases.append(("mix", lambda: engine.mix_round(W, X, Y, G=G, lr=LR, workspace=ws,
                                                      tiled=tiled)))
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
    out = {"case": f"K{n} {layout}", "agents": n, "params": P, "plan": plan,
           "mix_plan": mix_plan if mix_ok else None, **res}
    sec = res["dense"]["median_ms"] / 1e3
    out["dense_TBs_at_12B"] = round(12 * n * P / sec / 1e12, 3)
    out["dense_TFLOPs"] = round(2.0 * n * n * P / sec / 1e12, 2)
    if mix_ok:
        out["mix_TBs_at_12B"] = round(12 * n * P / (res["mix"]["median_ms"] / 1e3) / 1e12, 3)
        out["dense_vs_mix"] = {
            "ratio": round(res["dense"]["median_ms"] / res["mix"]["median_ms"], 4),
            "spread_ms": max(res["dense"]["block_spread_ms"], res["mix"]["block_spread_ms"])}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", default="64,128,256")
    ap.add_argument("--params", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="tiled,rows")
    ap.add_argument("--limit", type=int, default=120, help="seconds a case may take")
    ap.add_argument("--case", default=None, help="N,layout: run this one case in this process")
    args = ap.parse_args()
    if args.case:
        if not torch.cuda.is_available():
            raise SystemExit("dense_round_probe measures on the GPU; none is available")
        n, layout = args.case.split(",")
        probe(torch.device("cuda", 0), int(n), args.params, layout, args.rounds, args.blocks,
              args.warmup)
        return
    for n in [v for v in args.agents.split(",") if v]:
        for layout in [v for v in args.layouts.split(",") if v]:
            cmd = [sys.executable, os.path.abspath(__file__), "--case", f"{n},{layout}",
                   "--params", str(args.params), "--rounds", str(args.rounds),
                   "--blocks", str(args.blocks), "--warmup", str(args.warmup)]
            rc = subprocess.run(cmd, timeout=args.limit).returncode
            if rc != 0:   # a failed case ends the probe: nothing more is started on the device
                raise SystemExit(f"case {n},{layout} ended with status {rc}")


if __name__ == "__main__":
    main()
