"""dl_batch_gather at the c3 shape against what a user must do without it, and what it adds to
the captured c3 step: 256 agents x 64 samples x 784 floats per step from a 60000 x 784 dataset
resident in HBM (51.4 MB read, 51.4 MB written).

One process, one timed region per variant, variants interleaved, one HIP-event pair per call
after warm-up, medians over --samples each:
  gather            BatchSampler.next_into: one dl_batch_gather launch + the one-thread cursor step
  torch             the parent commit's way: slice the step's ids out of the table,
                    torch.index_select for data and labels, copy both into the static buffers
  torch_out         the leanest torch spelling, for information: index_select(out=) straight into
                    the static buffers (still a table slice from the host, no device cursor)
Then the captured c3 step (gradients + fused round with deviation, row-major as bench.py runs
it) with the sampler and with one fixed batch, alternating groups of --group replays, each group
between one event pair: median step time of both and their difference.

  python scripts/batch_gather_probe.py [--samples 50 --groups 20 --group 50]

One JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_learning_amd import engine  # noqa: E402
from distributed_learning_amd.graph import from_edge_weights, random_regular_edges  # noqa: E402
from distributed_learning_amd.networks.batched_ann import BatchedANN  # noqa: E402
from distributed_learning_amd.workloads import BatchSampler, MLPConsensusSGD  # noqa: E402


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
    ap.add_argument("--agents", type=int, default=256)
    ap.add_argument("--dataset", type=int, default=60000)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--group", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batch_gather_probe measures on the GPU; none is available")
    dev = torch.device("cuda", 0)
    n, B, din, dh, dout = args.agents, 64, 784, 150, 10
    gen = torch.Generator(device=dev).manual_seed(0)
    samples = torch.randn(args.dataset, din, device=dev, generator=gen)
    targets = torch.randint(0, dout, (args.dataset,), device=dev, generator=gen,
                            dtype=torch.int32)
    sampler = BatchSampler(samples, targets, n, B, seed=0)
    steps, table = sampler.steps, sampler.table
    data = torch.empty(n, B, din, device=dev)
    labels = torch.empty(n, B, device=dev, dtype=torch.int32)
    data2, labels2 = torch.empty_like(data), torch.empty_like(labels)
    host_step = [0]

    def ids_of_step():
        s = host_step[0]
        host_step[0] = (s + 1) % steps
        return table[:, s * B:(s + 1) * B].reshape(-1)

    def torch_path():
        ids = ids_of_step()
        data2.view(-1, din).copy_(samples.index_select(0, ids))
        labels2.view(-1).copy_(targets.index_select(0, ids))

    def torch_out_path():
        ids = ids_of_step()
        torch.index_select(samples, 0, ids, out=data2.view(-1, din))
        torch.index_select(targets, 0, ids, out=labels2.view(-1))

    cases = [("gather", lambda: sampler.next_into(data, labels)), ("torch", torch_path),
             ("torch_out", torch_out_path)]
    # the three agree (same table, same step) before anything is timed
    sampler.next_into(data, labels)
    torch_path()
    assert torch.equal(data, data2) and torch.equal(labels, labels2)
    sampler.cursor.zero_()
    host_step[0] = 0
    for _ in range(args.warmup):
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    ev = {name: [] for name, _ in cases}
    for _ in range(args.samples):
        for name, fn in cases:       # interleaved: every variant sees the same machine state
            ev[name].append(timed(fn))
    torch.cuda.synchronize()
    res = {name: summary([1e3 * s.elapsed_time(e) for s, e in v]) for name, v in ev.items()}
    moved = 2 * n * B * din * 4
    res["gather"]["gb_per_s"] = round(moved / (res["gather"]["median_us"] * 1e-6) / 1e9, 1)

    # the captured c3 step, sampler against one fixed batch
    edges = random_regular_edges(4, n, seed=0)
    csr = from_edge_weights(edges, [0.2] * len(edges), list(range(n)))
    runs = {}
    for name in ("fixed", "sampler"):
        ann = BatchedANN(n, B, din, dh, dout, device=dev)
        P_pad = MLPConsensusSGD.padded_params(csr, ann.P, dev)
        X0 = torch.zeros(n, P_pad, device=dev)
        X0[:, :ann.P] = 0.05 * torch.randn(n, ann.P, device=dev,
                                           generator=torch.Generator(device=dev).manual_seed(1))
        eng = engine.GossipEngine(csr, P_pad, device=dev, X=X0, layout="rows")
        if name == "sampler":
            sgd = MLPConsensusSGD(ann, eng, None, None, 0.05, sampler=sampler)
        else:
            ids = sampler.batch_ids(0)
            sgd = MLPConsensusSGD(ann, eng, samples[ids].contiguous(),
                                  targets[ids].contiguous(), 0.05)
        for _ in range(2):
            sgd.step()
        sgd.capture()
        sgd.replay(2 * args.warmup)
        runs[name] = sgd
    torch.cuda.synchronize()
    gev = {name: [] for name in runs}
    for _ in range(args.groups):
        for name, sgd in runs.items():
            gev[name].append(timed(lambda sgd=sgd: sgd.replay(args.group)))
    torch.cuda.synchronize()
    step = {name: summary([1e3 * s.elapsed_time(e) / args.group for s, e in v])
            for name, v in gev.items()}
    out = {"case": "c3 batch gather", "agents": n, "batch": B, "dim": din,
           "dataset_rows": args.dataset, "steps_per_epoch": steps, "bytes_moved": moved,
           **res,
           "gather_over_torch": round(res["gather"]["median_us"] / res["torch"]["median_us"], 4),
           "c3_step_fixed": step["fixed"], "c3_step_sampler": step["sampler"],
           "added_us_per_step": round(step["sampler"]["median_us"] - step["fixed"]["median_us"],
                                      2),
           "replays_per_group": args.group}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
