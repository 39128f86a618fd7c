"""The fused Chebyshev round (dl_cheb_round, y == z) against the two launches it replaces
(dl_mix_round into a scratch S, then dl_axpby of S and z into z), at the c2 shape: 1024 agents x
2^20 params on random_regular_graph(4, 1024, seed=0), row-major and column-tiled.

The two forms, the fused round with the deviation, and the triad in the round's access shape
(dl_stream_copy variant 6, 12 B per element) run interleaved in one process, one HIP-event pair
per round after warm-up; medians over --rounds samples each.  First the two forms run once from
the same X and Z and their outputs are compared bit for bit.

  python scripts/cheb_round_probe.py [--agents 1024 --params 1048576 --rounds 30]
  python scripts/cheb_round_probe.py --loop [--loop-params 4096 --loop-eps 1e-3]
      rounds and wall time to a fixed eps of the plain loop (round + 4-byte readback, Mixer.mix's
      round loop) against GossipEngine.mix_chebyshev on the 64 x 64 torus with the committed FDLA
      weights (tests/golden/fdla_torus64.npz), gamma from spectral_gamma

One JSON line per case."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from distributed_learning_amd import _lib, engine  # noqa: E402
import bench  # noqa: E402

A, B = 1.7, -0.7   # a late round's coefficients at gamma ~ 0.99


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
    X, Z = eng.X, eng.Y
    S, Z2 = eng._empty(), eng._empty()
    gen = torch.Generator(device=dev).manual_seed(0)
    for t in (X, Z):
        t.normal_(generator=gen)
    Z2.copy_(Z)
    flat = (lambda t: t.view(1, -1)) if tiled else (lambda t: t)
    kw = dict(workspace=eng.ws, tiled=tiled)
    plan = engine.cheb_round_plan(eng.W, X, Z, Z, deviation=True, tiled=tiled)
    if plan is None:
        raise SystemExit("the fused round does not take this shape")

    def two_launch():
        engine.mix_round(eng.W, X, S, **kw)
        engine.axpby(flat(S), flat(Z2), A, B, out=flat(Z2))

    def fused():
        assert engine.cheb_round(eng.W, X, Z, Z, A, B, **kw)

    def fused_dev():
        assert engine.cheb_round(eng.W, X, Z, Z, A, B, dev_sq=eng.dev_sq, dev_max=eng.dev_max, **kw)

    # same results first (the timed rounds below keep rewriting z, which stays bounded as |b| < 1:
    # only their time is used)
    two_launch()
    fused()
    torch.cuda.synchronize()
    same = bool(torch.equal(Z, Z2))

    lib = _lib.load()
    src = torch.zeros(2 * n * P, dtype=torch.float32, device=dev)
    dst = torch.empty(n * P, dtype=torch.float32, device=dev)

    def triad():
        _lib.check(lib.dl_stream_copy(_lib.ptr(src), _lib.ptr(dst), n * P, 6,
                                      _lib.stream_handle(dev)), "dl_stream_copy")

    cases = [("two_launch", two_launch), ("fused", fused), ("fused_dev", fused_dev),
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
        **{k: v for k, v in res.items()},
        "ratio_two_over_fused": round(two["median_ms"] / fu["median_ms"], 4),
        "ratio_two_over_fused_dev": round(two["median_ms"] / res["fused_dev"]["median_ms"], 4),
        "two_launch_spread_ms": round(two["p90_ms"] - two["p10_ms"], 4),
        "gain_ms": round(two["median_ms"] - fu["median_ms"], 4),
        "beats_spread": two["median_ms"] - fu["median_ms"] > two["max_ms"] - two["min_ms"],
        "fused_GBs_at_12B": round(12 * el / (fu["median_ms"] / 1e3) / 1e9, 1),
        "fused_dev_GBs_at_12B": round(12 * el / (res["fused_dev"]["median_ms"] / 1e3) / 1e9, 1),
        "two_launch_GBs_at_20B": round(20 * el / (two["median_ms"] / 1e3) / 1e9, 1),
        "triad6_GBs_at_12B": round(12 * el / (res["triad6"]["median_ms"] / 1e3) / 1e9, 1),
    }
    print(json.dumps(out), flush=True)


def probe_loop(dev, P, eps, max_rounds):
    from distributed_learning_amd.graph import first_appearance_vertices, from_edge_weights
    from distributed_learning_amd.utils.fast_averaging import spectral_gamma
    d = np.load(os.path.join(ROOT, "tests", "golden", "fdla_torus64.npz"))
    edges = [tuple(int(x) for x in e) for e in d["edges"]]
    verts = sorted(first_appearance_vertices(edges))
    csr = from_edge_weights(edges, d["w"], verts)
    gamma = spectral_gamma(edges, d["w"], verts)
    n = csr.n_rows
    X0 = torch.randn(n, P, generator=torch.Generator().manual_seed(0)).to(dev)
    eng = engine.GossipEngine(csr, P, device=dev, X=X0)
    tiled = (P, eng.T) if eng.layout == "tiled" else None
    fused = engine.cheb_round_plan(eng.W, eng.X, eng.Y, eng.Y, deviation=True,
                                   tiled=tiled) is not None

    def plain():
        done = 0
        while done < max_rounds:
            eng.round(deviation=True)
            done += 1
            if np.float32(eng.dev_max.item()) < eps:
                break
        return done

    out = {"case": "loop torus64 fdla", "agents": n, "params": P, "gamma": round(gamma, 8),
           "eps": eps, "layout": eng.layout, "path": eng.plan()["path"],
           "cheb_round": "fused" if fused else "dl_mix_round + dl_axpby"}

    def cheb():
        seen = []

        def guard(d):     # a loop that stalls above eps must end
            seen.append(d)
            if len(seen) > max_rounds:
                raise SystemExit(f"no convergence in {max_rounds} rounds (last {d})")
        return eng.mix_chebyshev(gamma, 1, eps, on_deviation=guard)

    for name, fn in (("plain", plain), ("chebyshev", cheb)):
        for rep in range(2):         # the second run is the timed one
            eng.load_rows(X0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        out[name] = {"rounds": k, "wall_ms": round(dt * 1e3, 2),
                     "final_max_dev": float(eng.dev_max.item())}
    out["round_ratio"] = round(out["plain"]["rounds"] / out["chebyshev"]["rounds"], 2)
    out["wall_ratio"] = round(out["plain"]["wall_ms"] / out["chebyshev"]["wall_ms"], 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--params", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layouts", default="rows,tiled")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--loop-params", type=int, default=4096)
    ap.add_argument("--loop-eps", type=float, default=1e-3)
    ap.add_argument("--loop-max-rounds", type=int, default=20000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cheb_round_probe measures on the GPU; none is available")
    dev = torch.device("cuda", 0)
    if args.loop:
        probe_loop(dev, args.loop_params, args.loop_eps, args.loop_max_rounds)
        return
    csr, _ = bench.build_graph(args.agents)
    for layout in [v for v in args.layouts.split(",") if v]:
        probe_layout(dev, csr, args.agents, args.params, layout, args.rounds, args.warmup)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
