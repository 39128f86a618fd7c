"""The fused Adam round (dl_adam_round, x' apart, m and v in place) against the composed form it
replaces -- dl_adam_step into a scratch S, dl_mix_round of S into Y -- at the c2 shape: 1024
agents x 2^20 params on random_regular_graph(4, 1024, seed=0), row-major and column-tiled, with
and without the deviation.

The composed form, the fused round, both with the deviation, and the triad in the round's access
shape (dl_stream_copy variant 6, 12 B per element) run interleaved in one process, one HIP-event
pair per round after warm-up.  The samples are taken in --blocks blocks of --rounds each; every
form's median is reported per block and overall, and the spread between a form's block medians
is the yardstick a gain must exceed.  First the two forms run once from the same X, G, M and V
and their outputs are compared bit for bit.

  python scripts/adam_round_probe.py [--agents 1024 --params 1048576 --rounds 20 --blocks 3]

One JSON line per layout."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from distributed_learning_amd import _lib, engine  # noqa: E402
import bench  # noqa: E402

LR = 1e-3
TICKS = 10    # the bias corrections of the tenth step, by value


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    return s, e


def summary(ms, blocks):
    """Overall median and range, and the median of each block of samples."""
    per = len(ms) // blocks
    meds = [statistics.median(ms[b * per:(b + 1) * per]) for b in range(blocks)]
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "block_medians_ms": [round(m, 4) for m in meds],
            "block_spread_ms": round(max(meds) - min(meds), 4), "samples": len(ms)}


def probe_layout(dev, csr, n, P, layout, rounds, blocks, warmup):
    eng = engine.GossipEngine(csr, P, device=dev, layout=layout)
    tiled = (P, eng.T) if eng.layout == "tiled" else None
    X, Y = eng.X, eng.Y
    G, M, V, S, M2, V2, Y2 = (eng._empty() for _ in range(7))
    gen = torch.Generator(device=dev).manual_seed(0)
    for t in (X, G, M):
        t.normal_(generator=gen)
    V.uniform_(0.0, 1.0, generator=gen)
    M2.copy_(M)
    V2.copy_(V)
    st = engine.AdamState(LR)
    for _ in range(TICKS):
        st.advance_host()
    opt = dict(lr=LR, step_size=st.step_size, bias2_sqrt=st.bias2_sqrt)
    kw = dict(workspace=eng.ws, tiled=tiled)
    dv = dict(dev_sq=eng.dev_sq, dev_max=eng.dev_max)
    plan = engine.adam_round_plan(eng.W, X, Y, G, M, V, deviation=True, tiled=tiled)
    if plan is None:
        raise SystemExit("the fused round does not take this shape")
    # a resident buffer is contiguous: the element-wise step sees it as one row
    flat = lambda t: t.view(1, -1)   # noqa: E731

    def composed(**dev_kw):
        engine.adam_step(flat(X), flat(G), flat(M2), flat(V2), out=flat(S), **opt)
        engine.mix_round(eng.W, S, Y2, **dev_kw, **kw)

    def fused(**dev_kw):
        assert engine.adam_round(eng.W, X, Y, G, M, V, **opt, **dev_kw, **kw)

    # same results first (the timed rounds below keep stepping m and v with the same gradient,
    # which converge: only their time is used)
    composed()
    fused()
    torch.cuda.synchronize()
    same = bool(torch.equal(M, M2) and torch.equal(V, V2) and torch.equal(Y, Y2))

    lib = _lib.load()
    src = torch.zeros(2 * n * P, dtype=torch.float32, device=dev)
    dst = torch.empty(n * P, dtype=torch.float32, device=dev)

    def triad():
        _lib.check(lib.dl_stream_copy(_lib.ptr(src), _lib.ptr(dst), n * P, 6,
                                      _lib.stream_handle(dev)), "dl_stream_copy")

    cases = [("composed", composed), ("fused", fused), ("composed_dev", lambda: composed(**dv)),
             ("fused_dev", lambda: fused(**dv)), ("triad6", triad)]
    for _ in range(warmup):
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    ev = {name: [] for name, _ in cases}
    for _ in range(rounds * blocks):
        for name, fn in cases:       # interleaved: every form sees the same machine state
            ev[name].append(timed(fn))
    torch.cuda.synchronize()
    res = {name: summary([s.elapsed_time(e) for s, e in v], blocks) for name, v in ev.items()}
    el = n * P
    tbs = lambda nbytes, r: round(nbytes * el / (r["median_ms"] / 1e3) / 1e12, 3)  # noqa: E731
    triad_tbs = tbs(12, res["triad6"])
    out = {"case": f"c2 {eng.layout}", "agents": n, "params": P, "plan": plan, "bit_equal": same,
           **res, "triad6_TBs_at_12B": triad_tbs}
    for f, c in (("fused", "composed"), ("fused_dev", "composed_dev")):
        gain = res[c]["median_ms"] - res[f]["median_ms"]
        spread = max(res[c]["block_spread_ms"], res[f]["block_spread_ms"])
        out[f + "_vs_" + c] = {
            "ratio": round(res[c]["median_ms"] / res[f]["median_ms"], 4),
            "gain_ms": round(gain, 4), "spread_ms": spread, "beats_spread": gain > spread,
            "fused_TBs_at_28B": tbs(28, res[f]),
            "fused_fraction_of_triad": round(tbs(28, res[f]) / triad_tbs, 4),
            "composed_TBs_at_36B": tbs(36, res[c])}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--params", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layouts", default="rows,tiled")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_round_probe measures on the GPU; none is available")
    dev = torch.device("cuda", 0)
    csr, _ = bench.build_graph(args.agents)
    for layout in [v for v in args.layouts.split(",") if v]:
        probe_layout(dev, csr, args.agents, args.params, layout, args.rounds, args.blocks,
                     args.warmup)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
