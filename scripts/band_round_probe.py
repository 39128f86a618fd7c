"""The banded round (dl_band_round, with g) against the plain round (dl_mix_round, with g) on the
same torus with one uniform edge weight:

  torus128,rows   128 x 128 agents x 2^16 params, row-major: dl_mix_round is the gather kernel
                  (plan path 2) -- the shape the banded round exists for
  torus128,tiled  the same, column-tiled in 16-column tiles (the plain round has no tiled form
                  here: the banded round alone)
  torus64,tiled   the 64 x 64 c4 torus x 2^18 in 4-column tiles, windows forced to a quarter of
                  the agents, against the register-CSR tile round (plan path 4): what the windows
                  cost where both kernels run

The byte bound of the banded round is (8 amplification + 4) B per element (x and g read once per
window, y written once) at the process's triad rate (c = a + s b over 2^28 floats, measured in
the same process).  The forms run interleaved, one HIP-event pair per round after warm-up, in
--blocks blocks of --rounds; the spread between a form's block medians is the yardstick a
difference must exceed.  Every case runs in a child process of its own under --limit seconds, and
the first case that fails or runs out of time ends the probe.

  python scripts/band_round_probe.py [--cases torus128,rows:torus128,tiled:torus64,tiled]

One JSON line per case."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from distributed_learning_amd import engine, graph  # noqa: E402

LR = 0.05
CASES = {"torus128": (128, 1 << 16, 16, None), "torus64": (64, 1 << 18, 4, 1024)}


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
            "block_medians_ms": [round(m, 4) for m in meds],
            "block_spread_ms": round(max(meds) - min(meds), 4), "samples": len(ms)}


def triad_rate(dev):
    """Bytes per second of c = a + s b over 2^28 floats (12 B an element), median of 10."""
    a, b, c = (torch.ones(1 << 28, device=dev) for _ in range(3))
    ev = [timed(lambda: torch.add(a, b, alpha=LR, out=c)) for _ in range(13)][3:]
    torch.cuda.synchronize()
    return 12.0 * a.numel() / (statistics.median(s.elapsed_time(e) for s, e in ev) / 1e3)


def probe(dev, name, layout, rounds, blocks, warmup):
    side, P, T, cap = CASES[name]
    n = side * side
    csr = graph.uniform_weights(graph.torus_edges(side, side), 0.2, list(range(n)))
    band = graph.band_blocks(csr, cap, tile_cols=T)
    tiled = layout == "tiled"
    triad = triad_rate(dev)
    eng = engine.GossipEngine(csr, P, device=dev, layout=layout, tile_cols=T if tiled else None,
                              order=None, band=band)
    gen = torch.Generator(device=dev).manual_seed(0)
    eng.X.copy_(torch.randn(eng.X.shape, device=dev, generator=gen))
    G = torch.randn(eng.X.shape, device=dev, generator=gen)
    plan = engine.band_round_plan(eng.W, eng._band, eng.X, eng.Y, G,
                                  tiled=(P, T) if tiled else None)
    cases = [("band", lambda: eng.round_band(G, LR))]
    mix_plan = None
    if not tiled or n <= 8192:      # the plain round serves this layout
        mix_plan = eng.plan(deviation=False)
        cases.append(("mix", lambda: eng.round(G, LR)))
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
    bound_ms = (8 * band.amplification + 4) * n * P / triad * 1e3
    out = {"case": f"{name} {layout}", "agents": n, "params": P, "tile_cols": T,
           "blocks": band.blocks, "max_window_rows": band.max_window_rows,
           "amplification": round(band.amplification, 4), "plan": plan, "mix_plan": mix_plan,
           "triad_TBs": round(triad / 1e12, 3), "byte_bound_ms": round(bound_ms, 4), **res,
           "band_fraction_of_bound": round(bound_ms / res["band"]["median_ms"], 3)}
    if "mix" in res:
        out["band_vs_mix"] = {
            "ratio": round(res["band"]["median_ms"] / res["mix"]["median_ms"], 4),
            "spread_ms": max(res["band"]["block_spread_ms"], res["mix"]["block_spread_ms"])}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="torus128,rows:torus128,tiled:torus64,tiled")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=150, help="seconds a case may take")
    ap.add_argument("--case", default=None, help="name,layout: run this one case in this process")
    args = ap.parse_args()
    if args.case:
        if not torch.cuda.is_available():
            raise SystemExit("band_round_probe measures on the GPU; none is available")
        name, layout = args.case.split(",")
        probe(torch.device("cuda", 0), name, layout, args.rounds, args.blocks, args.warmup)
        return
    for case in [v for v in args.cases.split(":") if v]:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--rounds",
               str(args.rounds), "--blocks", str(args.blocks), "--warmup", str(args.warmup)]
        rc = subprocess.run(cmd, timeout=args.limit).returncode
        if rc != 0:   # a failed case ends the probe: nothing more is started on the device
            raise SystemExit(f"case {case} ended with status {rc}")


if __name__ == "__main__":
    main()
