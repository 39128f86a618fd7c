"""The fused momentum-SGD round (dl_sgd_round) against the two launches it replaces
(dl_sgd_step into a scratch S, then dl_mix_round of S), at the c2 shape: 1024 agents x 2^20
params on random_regular_graph(4, 1024, seed=0), with the deviation, momentum 0.9, weight decay
5e-4, row-major and column-tiled.

The two forms, the fused round in place, and the triad in the round's access shape
(dl_stream_copy variant 6, 12 B per element) run interleaved in one process, one HIP-event pair
per round after warm-up; medians over --rounds samples each.  First the two forms run once from
the same X, G and M and their outputs are compared bit for bit.

  python scripts/sgd_round_probe.py [--agents 1024 --params 1048576 --rounds 30]
  python scripts/sgd_round_probe.py --c5 [--c5-agents 8 --c5-batch 16 --c5-steps 10]
      the c5 workload's step time with fused_round off and on (hipGraph replays, interleaved)

One JSON line per case."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_learning_amd import _lib, engine  # noqa: E402
from distributed_learning_amd.workloads import WRNConsensusSGD, sgd_step  # noqa: E402
import bench  # noqa: E402

OPT = dict(momentum=0.9, weight_decay=5e-4)
LR = 0.02


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    return s, e


def summary(ms):
    ms = sorted(ms)
    q = statistics.quantiles(ms, n=10)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4),
            "max_ms": round(ms[-1], 4), "p10_ms": round(q[0], 4), "p90_ms": round(q[-1], 4),
            "samples": len(ms)}


def probe_layout(dev, csr, n, P, layout, rounds, warmup):
    eng = engine.GossipEngine(csr, P, device=dev, layout=layout)
    tiled = (P, eng.T) if eng.layout == "tiled" else None
    X, Y = eng.X, eng.Y
    G, M, S = eng._empty(), eng._empty(), eng._empty()
    gen = torch.Generator(device=dev).manual_seed(0)
    for t in (X, G, M):
        t.normal_(generator=gen)
    flat = (lambda t: t.view(1, -1)) if tiled else (lambda t: t)
    kw = dict(dev_sq=eng.dev_sq, dev_max=eng.dev_max, workspace=eng.ws, tiled=tiled)
    plan = engine.sgd_round_plan(eng.W, X, Y, G, M, deviation=True, tiled=tiled, **OPT)
    if plan is None:
        raise SystemExit("the fused round does not take this shape")

    def two_launch():
        sgd_step(flat(X), flat(G), flat(M), out=flat(S), lr=LR, **OPT)
        engine.mix_round(eng.W, S, Y, **kw)

    def fused():
        assert engine.sgd_round(eng.W, X, Y, G, M, LR, **OPT, **kw)

    def fused_in_place():
        assert engine.sgd_round(eng.W, X, X, G, M, LR, **OPT, **kw)

    # same results first (the timed rounds below keep stepping M: only their time is used)
    M0 = M.clone()
    two_launch()
    Ya, Ma, da = Y.clone(), M.clone(), eng.dev_sq.clone()
    M.copy_(M0)
    fused()
    torch.cuda.synchronize()
    same = bool(torch.equal(Ya, Y) and torch.equal(Ma, M))
    dev_rel = float(((eng.dev_sq - da).abs() / da.abs().clamp_min(1e-30)).max())
    del Ya, Ma, M0

    lib = _lib.load()
    src = torch.zeros(2 * n * P, dtype=torch.float32, device=dev)
    dst = torch.empty(n * P, dtype=torch.float32, device=dev)

    def triad():
        _lib.check(lib.dl_stream_copy(_lib.ptr(src), _lib.ptr(dst), n * P, 6,
                                      _lib.stream_handle(dev)), "dl_stream_copy")

    cases = [("two_launch", two_launch), ("fused", fused), ("fused_in_place", fused_in_place),
             ("triad6", triad)]
    for _ in range(warmup):
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    ev = {name: [] for name, _ in cases}
    for _ in range(rounds):
        for name, fn in cases:       # interleaved: every form sees the same machine state
            ev[name].append(timed(fn))
    torch.cuda.synchronize()
    res = {name: summary([s.elapsed_time(e) for s, e in v]) for name, v in ev.items()}
    el = n * P
    two, fu = res["two_launch"], res["fused"]
    out = {
        "case": f"c2 {eng.layout}", "agents": n, "params": P, "plan": plan, "bit_equal": same,
        "dev_sq_max_rel_diff": dev_rel, **{k: v for k, v in res.items()},
        "ratio_two_over_fused": round(two["median_ms"] / fu["median_ms"], 4),
        "ratio_two_over_fused_in_place": round(two["median_ms"] /
                                               res["fused_in_place"]["median_ms"], 4),
        "two_launch_spread_ms": round(two["p90_ms"] - two["p10_ms"], 4),
        "gain_ms": round(two["median_ms"] - fu["median_ms"], 4),
        "beats_spread": two["median_ms"] - fu["median_ms"] > two["max_ms"] - two["min_ms"],
        "fused_GBs_at_20B": round(20 * el / (fu["median_ms"] / 1e3) / 1e9, 1),
        "fused_in_place_GBs_at_20B": round(20 * el / (res["fused_in_place"]["median_ms"] / 1e3)
                                           / 1e9, 1),
        "two_launch_GBs_at_28B": round(28 * el / (two["median_ms"] / 1e3) / 1e9, 1),
        "triad6_GBs_at_12B": round(12 * el / (res["triad6"]["median_ms"] / 1e3) / 1e9, 1),
    }
    print(json.dumps(out), flush=True)


def probe_c5(dev, n, batch, steps, warmup):
    csr, _ = bench.build_graph(n)
    wl = {f: WRNConsensusSGD(csr, batch, device=dev, seed=0, fused_round=f) for f in (False, True)}
    assert wl[True].fused_round and wl[True].S is None
    for w in wl.values():
        for _ in range(2):
            w.step()
        w.capture()
        w.replay(warmup)
    torch.cuda.synchronize()
    ev = {f: [] for f in wl}
    for _ in range(steps):
        for f, w in wl.items():
            ev[f].append(timed(lambda: w.replay(1)))
    torch.cuda.synchronize()
    res = {("fused" if f else "two_launch"): summary([s.elapsed_time(e) for s, e in v])
           for f, v in ev.items()}
    print(json.dumps({"case": "c5 step", "agents": n, "batch": batch, "params": wl[True].P,
                      "resident_matrices": {"two_launch": 5, "fused": 4}, **res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--params", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layouts", default="rows,tiled")
    ap.add_argument("--c5", action="store_true")
    ap.add_argument("--c5-agents", type=int, default=8)
    ap.add_argument("--c5-batch", type=int, default=16)
    ap.add_argument("--c5-steps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sgd_round_probe measures on the GPU; none is available")
    dev = torch.device("cuda", 0)
    if args.c5:
        probe_c5(dev, args.c5_agents, args.c5_batch, args.c5_steps, args.warmup)
        return
    csr, _ = bench.build_graph(args.agents)
    for layout in [v for v in args.layouts.split(",") if v]:
        probe_layout(dev, csr, args.agents, args.params, layout, args.rounds, args.warmup)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
