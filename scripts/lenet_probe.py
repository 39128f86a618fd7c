"""dl_lenet_grad at the reference's LeNet shape against what a user has without it.

  64 agents x batch 64 x 10 classes, randn images, torch's default init per agent

One process, variants interleaved, one HIP-event pair per call after warm-up, medians over
--samples each:
  lenet_grad    BatchedLeNet.gradients: one dl_lenet_grad call (its fixed sequence of launches)
  module_loop   the loop WRNConsensusSGD._local_grads runs, with a LeNet module per agent whose
                parameters and gradients are views of the rows of X and G: zero G, then per agent
                forward, cross_entropy, backward (PyTorch / MIOpen, one stream)
Then the call's launches one by one: dl_lenet_grad_events records an event before each launch
and one after the last; medians of the gaps over --samples calls.

  python scripts/lenet_probe.py [--agents 64 --batch 64 --samples 30 --out probe.json]

One JSON line (also written to --out when given)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_learning_amd import _lib  # noqa: E402
from distributed_learning_amd.networks.batched_lenet import BatchedLeNet  # noqa: E402
from distributed_learning_amd.networks.lenet import LeNet  # noqa: E402

LAUNCHES = ["conv_fwd", "fc1", "fc2", "fc3_xent", "dW_fc3", "dZ_fc2", "dW_fc2", "dZ_fc1",
            "dW_fc1", "d_pool2", "conv_bwd", "conv_reduce"]


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    return s, e


def summary(us):
    us = sorted(us)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(us[0], 2),
            "max_us": round(us[-1], 2), "samples": len(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lenet_probe measures on the GPU; none is available")
    if args.batch > 64:
        raise SystemExit("the launch names below are those of batch <= 64")
    dev = torch.device("cuda", 0)
    N, B, nc = args.agents, args.batch, args.classes
    net = BatchedLeNet(N, B, nc, device=dev)
    P, ld = net.P, -(-net.P // 64) * 64
    Xb = torch.zeros(N, ld, device=dev)
    Gb, Gl = torch.zeros_like(Xb), torch.zeros_like(Xb)
    X, G = Xb[:, :P], Gb[:, :P]
    models = []
    for a in range(N):
        torch.manual_seed(a)
        m = LeNet(nc).to(dev)
        with torch.no_grad():
            X[a] = torch.cat([p.reshape(-1) for p in m.parameters()])
            off = 0
            for p in m.parameters():   # as WRNConsensusSGD: parameters and gradients are row views
                n = p.numel()
                p.set_(Xb[a, off:off + n].view_as(p))
                p.grad = Gl[a, off:off + n].view_as(p)
                off += n
        models.append(m)
    g = torch.Generator(device=dev).manual_seed(0)
    data = torch.randn(N, B, 3, 32, 32, device=dev, generator=g)
    labels = torch.randint(0, nc, (N, B), device=dev, generator=g)
    labels32 = labels.int()
    loop_loss = torch.zeros(N, device=dev)

    def module_loop():
        Gl.zero_()
        for a, m in enumerate(models):
            loss = F.cross_entropy(m(data[a]), labels[a])
            loss.backward()
            loop_loss[a:a + 1].copy_(loss.detach().reshape(1))

    def lenet_grad():
        net.gradients(X, data, labels32, G)

    # the two agree before anything is timed
    lenet_grad()
    module_loop()
    torch.cuda.synchronize()
    scale = Gl[:, :P].abs().max()
    agree = float((G - Gl[:, :P]).abs().max() / scale)
    assert agree < 1e-4, agree
    cases = [("lenet_grad", lenet_grad), ("module_loop", module_loop)]
    for _ in range(args.warmup):
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k, _ in cases}
    for _ in range(args.samples):
        for k, fn in cases:          # interleaved: both see the same machine state
            ev[k].append(timed(fn))
    torch.cuda.synchronize()
    res = {k: summary([1e3 * s.elapsed_time(e) for s, e in v]) for k, v in ev.items()}

    # the call's launches one by one
    lib = _lib.load()
    need = lib.dl_lenet_workspace_bytes(N, B, nc)
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
    cargs = _lib.DlLenetArgs(N, B, nc, _lib.ptr(X), ld, _lib.ptr(data), B * 3072,
                             _lib.ptr(labels32), B, _lib.ptr(G), ld, _lib.ptr(net.loss), None, 0,
                             0)
    n_ev = len(LAUNCHES) + 1
    gaps = [[] for _ in LAUNCHES]
    sets = []
    for _ in range(args.samples):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n_ev)]
        for e in evs:
            e.record()               # creates the HIP event behind it
        handles = (ctypes.c_void_p * n_ev)(*[e.cuda_event for e in evs])
        n_launch = ctypes.c_int32(0)
        _lib.check(lib.dl_lenet_grad_events(ctypes.byref(cargs), _lib.ptr(ws), need,
                                            _lib.stream_handle(dev), handles, n_ev,
                                            ctypes.byref(n_launch)), "dl_lenet_grad_events")
        assert n_launch.value == len(LAUNCHES)
        sets.append(evs)
    torch.cuda.synchronize()
    for evs in sets:
        for i in range(len(LAUNCHES)):
            gaps[i].append(1e3 * evs[i].elapsed_time(evs[i + 1]))
    launches = {name: summary(v) for name, v in zip(LAUNCHES, gaps)}
    out = {"case": "lenet grad", "agents": N, "batch": B, "classes": nc, "params": P,
           "flops_per_call": net.flops_per_step(), **res,
           "max_abs_diff_over_max_grad": agree,
           "loop_over_lenet_grad": round(res["module_loop"]["median_us"] /
                                         res["lenet_grad"]["median_us"], 2),
           "gflops_per_s": round(net.flops_per_step() / res["lenet_grad"]["median_us"] / 1e3, 1),
           "launches": launches,
           "launch_sum_us": round(sum(v["median_us"] for v in launches.values()), 2)}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
