"""dl_lenet_eval at the reference's test shape against the path it replaces.

  64 agents x 10 000 shared rows x 10 classes, randn images, torch's default init per agent

One process, variants interleaved, HIP events around a span of --span calls after warm-up,
medians over --spans spans each, with the spread:
  fused     BatchedLeNet.evaluate(fused=True): one dl_lenet_eval call (two kernels)
  chunked   BatchedLeNet.evaluate(chunk=512): per chunk the forward-only dl_lenet_grad and the
            torch ops on its logits
Then the floor both share: the convolution forward launches alone (dl_lenet_grad_events, logits
only, chunks of 512 rows and the last chunk), summed over the test set.  Also the plan
(lds_bytes, row_splits, grid) and both workspaces' bytes.

  python scripts/lenet_eval_probe.py [--agents 64 --rows 10000 --spans 7 --out probe.json]

One JSON line (also written to --out when given)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_learning_amd import _lib  # noqa: E402
from distributed_learning_amd.networks.batched_lenet import BatchedLeNet  # noqa: E402
from distributed_learning_amd.networks.lenet import LeNet  # noqa: E402


def summary(ms):
    ms = sorted(ms)
    med = statistics.median(ms)
    return {"median_ms": round(med, 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
            "spread_pct": round(100 * (ms[-1] - ms[0]) / med, 2), "spans": len(ms)}


def conv_forward_us(lib, dev, X, ld, data, rows, nc, samples):
    """Median time of the convolution forward launch of a logits-only dl_lenet_grad on `rows`
    shared rows: the gap between the first two events of dl_lenet_grad_events."""
    N = X.shape[0]
    need = lib.dl_lenet_workspace_bytes(N, rows, nc)
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
    z = torch.empty(N, rows, nc, device=dev)
    cargs = _lib.DlLenetArgs(N, rows, nc, _lib.ptr(X), ld, _lib.ptr(data), 0, None, 0, None, 0,
                             None, _lib.ptr(z), nc, rows * nc)
    n_ev = 5                                  # conv, fc1, fc2, fc3 -> logits, and the end
    sets = []
    for _ in range(samples + 2):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n_ev)]
        for e in evs:
            e.record()                        # creates the HIP event behind it
        handles = (ctypes.c_void_p * n_ev)(*[e.cuda_event for e in evs])
        n_launch = ctypes.c_int32(0)
        _lib.check(lib.dl_lenet_grad_events(ctypes.byref(cargs), _lib.ptr(ws), need,
                                            _lib.stream_handle(dev), handles, n_ev,
                                            ctypes.byref(n_launch)), "dl_lenet_grad_events")
        assert n_launch.value == n_ev - 1
        sets.append(evs)
    torch.cuda.synchronize()
    return statistics.median(1e3 * evs[0].elapsed_time(evs[1]) for evs in sets[2:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--span", type=int, default=3, help="calls per timed span")
    ap.add_argument("--spans", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--row-splits", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.spans < 5:
        raise SystemExit("medians of at least five spans")
    if not torch.cuda.is_available():
        raise SystemExit("lenet_eval_probe measures on the GPU; none is available")
    dev = torch.device("cuda", 0)
    N, R, nc, chunk = args.agents, args.rows, args.classes, min(args.chunk, args.rows)
    net = BatchedLeNet(N, 64, nc, device=dev)
    P, ld = net.P, -(-net.P // 64) * 64
    Xb = torch.zeros(N, ld, device=dev)
    X = Xb[:, :P]
    for a in range(N):
        torch.manual_seed(a)
        X[a] = torch.cat([p.detach().reshape(-1) for p in LeNet(nc).parameters()]).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    data = torch.randn(R, 3, 32, 32, device=dev, generator=g)
    labels = torch.randint(0, nc, (R,), device=dev, generator=g).int()

    def fused():
        return net.evaluate(X, data, labels, fused=True, row_splits=args.row_splits)

    def chunked():
        return net.evaluate(X, data, labels, chunk=chunk, fused=False)

    # the two agree before anything is timed
    lf, cf = (t.clone() for t in fused())
    lc, cc = (t.clone() for t in chunked())
    torch.cuda.synchronize()
    loss_rel = float(((lf - lc).abs() / lc.abs()).max())
    assert loss_rel < 1e-5 and torch.equal(cf, cc), (loss_rel, cf, cc)
    cases = [("fused", fused), ("chunked", chunked)]
    for _ in range(args.warmup):
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k, _ in cases}
    for _ in range(args.spans):
        for k, fn in cases:                   # interleaved: both see the same machine state
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.span):
                fn()
            e.record()
            ev[k].append((s, e))
    torch.cuda.synchronize()
    res = {k: summary([s.elapsed_time(e) / args.span for s, e in v]) for k, v in ev.items()}

    lib = _lib.load()
    pl = _lib.DlLenetEvalPlan()
    pargs = _lib.DlLenetEvalArgs(N, R, nc, _lib.ptr(X), ld, _lib.ptr(data), 0, _lib.ptr(labels), 0,
                                 _lib.ptr(lf), _lib.ptr(cf), None, 0, 0, args.row_splits)
    _lib.check(lib.dl_lenet_eval_plan_query(ctypes.byref(pargs), ctypes.byref(pl)),
               "dl_lenet_eval_plan_query")
    # the floor: the convolution forward launches of the chunked path, summed over the test set
    full, last = divmod(R, chunk)
    conv_us = full * conv_forward_us(lib, dev, X, ld, data, chunk, nc, 10)
    if last:
        conv_us += conv_forward_us(lib, dev, X, ld, data, last, nc, 10)
    out = {"case": "lenet eval", "agents": N, "rows": R, "classes": nc, "chunk": chunk,
           "calls_per_span": args.span, **res,
           "fused_over_chunked": round(res["fused"]["median_ms"] / res["chunked"]["median_ms"], 3),
           "conv_forward_floor_ms": round(conv_us / 1e3, 3),
           "fused_over_conv_floor": round(res["fused"]["median_ms"] / (conv_us / 1e3), 3),
           "plan": {"blocks": pl.blocks, "row_splits": pl.row_splits, "grid": pl.grid,
                    "lds_bytes": pl.lds_bytes},
           "fused_workspace_bytes": int(lib.dl_lenet_eval_workspace_bytes(N, R)),
           "chunked_workspace_bytes": int(lib.dl_lenet_workspace_bytes(N, chunk, nc)),
           "loss_rel_diff": loss_rel, "correct_equal": True}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
