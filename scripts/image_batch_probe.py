"""dl_image_batch at the c5 and c3 shapes against what a user must do without it, and what it
costs in the captured steps.

  (a) c5: 64 agents x 64 x 3x32x32 from 50000 uint8 samples, pad 4, flip on
  (b) c3: 256 agents x 64 x 1x28x28 from 60000 uint8 samples, no augmentation

One process, variants interleaved, one HIP-event pair per call after warm-up, medians over
--samples each:
  image_batch   ImageBatchSampler.next_into: one dl_image_batch launch + the one-thread cursor step
  torch         a torch restatement into the same static buffers: slice the step's ids and draws
                out of the tables, index_select the uint8 rows, F.pad, crop and flip per sample by
                one advanced-indexing gather, the table lookup, labels likewise ((b): no pad, no
                crop -- index_select and the lookup)
  gather_fp32   (b) only: BatchSampler.next_into = dl_batch_gather on the fp32 copy of the data
Then the captured steps, alternating groups of replays between one event pair each:
  c3 (256 agents, as bench.py runs it): BatchSampler against ImageBatchSampler
  c5 (WRN-16-4, 8 agents on a ring, B = 64): one fixed batch against the sampler

  python scripts/image_batch_probe.py [--samples 50 --groups 20 --group 50 --no-c5]

One JSON line (also written to --out when given)."""
import argparse
import json
import os
import statistics
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_learning_amd import engine  # noqa: E402
from distributed_learning_amd.graph import (best_constant_weight, from_edge_weights,  # noqa: E402
                                            random_regular_edges, uniform_weights)
from distributed_learning_amd.networks.batched_ann import BatchedANN  # noqa: E402
from distributed_learning_amd.workloads import (BatchSampler, ImageBatchSampler,  # noqa: E402
                                                MLPConsensusSGD, WRNConsensusSGD)

MNIST = ((0.1307,), (0.3081,))
CIFAR = ((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))


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


def torch_restatement(sampler, data, labels):
    """The torch path for one step into static buffers, walking the epoch from the host."""
    dev, B, pad = sampler.device, sampler.batch, sampler.pad
    C, H, W = sampler.shape
    ch = torch.arange(C, device=dev).view(1, C, 1, 1)
    rows_y, cols_x = torch.arange(H, device=dev), torch.arange(W, device=dev)
    host_step = [0]

    def step():
        s = host_step[0]
        host_step[0] = (s + 1) % sampler.steps
        ids = sampler.table[:, s * B:(s + 1) * B].reshape(-1)
        rows = sampler.samples.index_select(0, ids)
        if pad or sampler.flip:
            w = sampler.aug[:, s * B:(s + 1) * B].reshape(-1)
            top, left, flip = (w & 255).view(-1, 1), ((w >> 8) & 255).view(-1, 1), \
                ((w >> 16) & 1).view(-1, 1).bool()
            padded = F.pad(rows, (pad, pad, pad, pad), value=sampler.fill)
            ys = (top + rows_y).view(-1, 1, H, 1)
            xs = (left + torch.where(flip, W - 1 - cols_x, cols_x)).view(-1, 1, 1, W)
            n = torch.arange(rows.shape[0], device=dev).view(-1, 1, 1, 1)
            rows = padded[n, ch, ys, xs]
        data.view(-1, C, H, W).copy_(sampler.lut[ch, rows.long()])
        labels.view(-1).copy_(sampler.targets.index_select(0, ids))
    return step, host_step


def launch_probe(name, sampler, args, extra=None):
    """Interleaved medians of next_into, the torch restatement and the extra variants."""
    dev, n, B = sampler.device, sampler.n_agents, sampler.batch
    data = torch.empty(n, B, *sampler.shape, device=dev)
    labels = torch.empty(n, B, device=dev, dtype=torch.int32)
    data2, labels2 = torch.empty_like(data), torch.empty_like(labels)
    torch_step, host_step = torch_restatement(sampler, data2, labels2)
    cases = [("image_batch", lambda: sampler.next_into(data, labels)), ("torch", torch_step)]
    cases += list((extra or {}).items())
    # the two agree (same tables, same step) before anything is timed
    sampler.cursor.zero_()
    for _ in range(2):
        sampler.next_into(data, labels)
        torch_step()
        assert torch.equal(data, data2) and torch.equal(labels, labels2)
    sampler.cursor.zero_()
    host_step[0] = 0
    for _ in range(args.warmup):
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k, _ in cases}
    for _ in range(args.samples):
        for k, fn in cases:          # interleaved: every variant sees the same machine state
            ev[k].append(timed(fn))
    torch.cuda.synchronize()
    res = {k: summary([1e3 * s.elapsed_time(e) for s, e in v]) for k, v in ev.items()}
    moved = n * B * sampler.dim * 5          # one byte read, four written per pixel
    res["image_batch"]["gb_per_s"] = round(moved / (res["image_batch"]["median_us"] * 1e-6) / 1e9,
                                           1)
    return {"shape": name, "agents": n, "batch": B, "image": list(sampler.shape),
            "dataset_samples": int(sampler.samples.shape[0]), "pad": sampler.pad,
            "flip": sampler.flip, "steps_per_epoch": sampler.steps, "bytes_moved": moved, **res,
            "image_batch_over_torch": round(res["image_batch"]["median_us"] /
                                            res["torch"]["median_us"], 4)}


def grouped(runs, groups, group):
    """Median time per step of each run, alternating groups of `group` replays."""
    torch.cuda.synchronize()
    gev = {k: [] for k in runs}
    for _ in range(groups):
        for k, wl in runs.items():
            gev[k].append(timed(lambda wl=wl: wl.replay(group)))
    torch.cuda.synchronize()
    return {k: summary([1e3 * s.elapsed_time(e) / group for s, e in v]) for k, v in gev.items()}


def c3_steps(dev, u8, f32, args):
    n, B, din, dh, dout = u8.n_agents, 64, 784, 150, 10
    edges = random_regular_edges(4, n, seed=0)
    csr = from_edge_weights(edges, [0.2] * len(edges), list(range(n)))
    runs = {}
    for name, sampler in (("batch_sampler_fp32", f32), ("image_batch_sampler_u8", u8)):
        ann = BatchedANN(n, B, din, dh, dout, device=dev)
        P_pad = MLPConsensusSGD.padded_params(csr, ann.P, dev)
        X0 = torch.zeros(n, P_pad, device=dev)
        X0[:, :ann.P] = 0.05 * torch.randn(n, ann.P, device=dev,
                                           generator=torch.Generator(device=dev).manual_seed(1))
        eng = engine.GossipEngine(csr, P_pad, device=dev, X=X0, layout="rows")
        sgd = MLPConsensusSGD(ann, eng, None, None, 0.05, sampler=sampler)
        for _ in range(2):
            sgd.step()
        sgd.capture()
        sgd.replay(2 * args.warmup)
        runs[name] = sgd
    return grouped(runs, args.groups, args.group)


def c5_steps(dev, args):
    n, B = 8, 64
    edges = [(i, (i + 1) % n) for i in range(n)]
    csr = uniform_weights(edges, best_constant_weight(edges))
    g = torch.Generator(device=dev).manual_seed(2)
    img = torch.randint(0, 256, (n * B * 4, 3, 32, 32), device=dev, generator=g,
                        dtype=torch.uint8)
    tg = torch.randint(0, 10, (img.shape[0],), device=dev, generator=g, dtype=torch.int32)
    sampler = ImageBatchSampler(img, tg, n, B, *CIFAR, pad=4, flip=True, seed=0)
    runs = {}
    for name, kw in (("fixed_batch", {}), ("image_batch_sampler", dict(sampler=sampler))):
        wl = WRNConsensusSGD(csr, B, device=dev, seed=0, streams=8, **kw)
        for _ in range(2):
            wl.step()
        wl.capture()
        wl.replay(3)
        runs[name] = wl
    return grouped(runs, args.c5_groups, args.c5_group)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--group", type=int, default=50)
    ap.add_argument("--c5-groups", type=int, default=8)
    ap.add_argument("--c5-group", type=int, default=5)
    ap.add_argument("--no-c5", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_batch_probe measures on the GPU; none is available")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    out = {"case": "image batch"}

    def emit():
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(out) + "\n")

    # (a) c5
    img = torch.randint(0, 256, (50000, 3, 32, 32), device=dev, generator=gen, dtype=torch.uint8)
    tg = torch.randint(0, 10, (50000,), device=dev, generator=gen, dtype=torch.int32)
    a = ImageBatchSampler(img, tg, 64, 64, *CIFAR, pad=4, flip=True, seed=0)
    out["c5_shape"] = launch_probe("c5", a, args)
    emit()
    del a, img, tg
    # (b) c3
    img = torch.randint(0, 256, (60000, 1, 28, 28), device=dev, generator=gen, dtype=torch.uint8)
    tg = torch.randint(0, 10, (60000,), device=dev, generator=gen, dtype=torch.int32)
    u8 = ImageBatchSampler(img, tg, 256, 64, *MNIST, seed=0)
    f32 = BatchSampler(u8.eval_transform(img), tg, 256, 64, seed=0)
    fdata = torch.empty(256, 64, 784, device=dev)
    flabels = torch.empty(256, 64, device=dev, dtype=torch.int32)
    out["c3_shape"] = launch_probe(
        "c3", u8, args, extra={"gather_fp32": lambda: f32.next_into(fdata, flabels)})
    out["c3_shape"]["image_batch_over_gather_fp32"] = round(
        out["c3_shape"]["image_batch"]["median_us"] /
        out["c3_shape"]["gather_fp32"]["median_us"], 4)
    out["c3_shape"]["dataset_bytes"] = {"uint8": img.numel(), "fp32": 4 * img.numel()}
    emit()
    step = c3_steps(dev, u8, f32, args)
    out["c3_step"] = {**step, "replays_per_group": args.group,
                      "u8_minus_fp32_us": round(step["image_batch_sampler_u8"]["median_us"] -
                                                step["batch_sampler_fp32"]["median_us"], 2)}
    emit()
    del u8, f32, img, tg, fdata, flabels
    if not args.no_c5:
        step = c5_steps(dev, args)
        out["c5_step_8_agents"] = {
            **step, "replays_per_group": args.c5_group,
            "added_us_per_step": round(step["image_batch_sampler"]["median_us"] -
                                       step["fixed_batch"]["median_us"], 2)}
        emit()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
