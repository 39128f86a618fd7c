"""The one-launch evaluation (dl_mlp_eval) against the gradient launch whose forward it shares,
at the c3 shape: 256 agents x ANNModel(784, 150, 10), one test set of R = 64 k rows shared by all
agents (k = 16 and k = 156 by default), parameters row-major or column-tiled.

dl_mlp_eval over 64 k rows and dl_mlp_grad over 64 rows per agent run interleaved in one process,
one HIP-event pair per launch after warm-up; medians over --samples each.  The forward is a
strict subset of the gradient's work on the same rows, so the evaluation must take less than k
gradient launches: ratio = eval / (k * grad) below 1.  Also the evaluation's effective TFLOP/s
(BatchedANN.eval_flops, the forward's FLOPs) and the row splits the plan chose.

  python scripts/mlp_eval_probe.py [--agents 256 --k 16,156 --samples 20 --layout tiled]

One JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_learning_amd import _lib, engine  # noqa: E402
from distributed_learning_amd.networks.batched_ann import BatchedANN  # noqa: E402


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    return s, e


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4),
            "max_ms": round(ms[-1], 4), "samples": len(ms)}


def plan(bann, X, rows, row_splits):
    tiled = X.dim() == 3
    a = _lib.DlMlpEvalArgs(bann.N, rows, bann.din, bann.dh, bann.dout, _lib.ptr(X),
                           0 if tiled else X.stride(0), X.shape[2] if tiled else 0,
                           ctypes.c_void_p(1 << 40), 0, ctypes.c_void_p(1 << 41), 0,
                           ctypes.c_void_p(1 << 42), None, None, 0, 0, row_splits)
    pl = _lib.DlMlpEvalPlan()
    _lib.check(_lib.load().dl_mlp_eval_plan_query(ctypes.byref(a), ctypes.byref(pl)),
               "dl_mlp_eval_plan_query")
    return {f: getattr(pl, f) for f, _ in pl._fields_}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=256)
    ap.add_argument("--k", default="16,156")
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layout", default="tiled", choices=["rows", "tiled"])
    ap.add_argument("--row-splits", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlp_eval_probe measures on the GPU; none is available")
    dev = torch.device("cuda", 0)
    n, din, dh, dout = args.agents, 784, 150, 10
    ks = [int(v) for v in args.k.split(",") if v]
    bann = BatchedANN(n, 64, din, dh, dout, device=dev, path="fused")
    gen = torch.Generator(device=dev).manual_seed(0)
    ld = -(-bann.P // 64) * 64
    X = torch.zeros(n, ld, device=dev)
    X[:, :bann.P] = 0.05 * torch.randn(n, bann.P, device=dev, generator=gen)
    if args.layout == "tiled":
        X = engine.to_tiled(X[:, :bann.P].contiguous(), 64)
        G = torch.empty_like(X)
    else:
        G = torch.empty_like(X)[:, :bann.P]
        X = X[:, :bann.P]
    train = torch.randn(n, 64, din, device=dev, generator=gen)
    train_lab = torch.randint(0, dout, (n, 64), device=dev, generator=gen, dtype=torch.int32)
    rmax = 64 * max(ks)
    test = torch.randn(rmax, din, device=dev, generator=gen)
    test_lab = torch.randint(0, dout, (rmax,), device=dev, generator=gen, dtype=torch.int32)

    cases = [("grad", lambda: bann.gradients(X, train, train_lab, G))]
    for k in ks:
        d, lab = test[:64 * k], test_lab[:64 * k]
        cases.append((f"eval_k{k}", lambda d=d, lab=lab: bann.evaluate(
            X, d, lab, row_splits=args.row_splits)))
    for _ in range(args.warmup):
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    ev = {name: [] for name, _ in cases}
    for _ in range(args.samples):
        for name, fn in cases:       # interleaved: every launch sees the same machine state
            ev[name].append(timed(fn))
    torch.cuda.synchronize()
    res = {name: summary([s.elapsed_time(e) for s, e in v]) for name, v in ev.items()}
    grad = res["grad"]["median_ms"]
    out = {"case": f"c3 eval {args.layout}", "agents": n, "dims": [din, dh, dout],
           "grad_64_rows": res["grad"]}
    for k in ks:
        r = res[f"eval_k{k}"]
        out[f"eval_k{k}"] = {
            **r, "rows": 64 * k, "plan": plan(bann, X, 64 * k, args.row_splits),
            "ratio_eval_over_k_grad": round(r["median_ms"] / (k * grad), 4),
            "tflops": round(bann.eval_flops(64 * k) / (r["median_ms"] / 1e3) / 1e12, 2)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
