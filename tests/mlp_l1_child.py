"""Child process of tests/test_mlp_x6_gpu.py::test_all_fp32_variant (a plain script, not
collected).  DLAMD_MLP_L1 is read once per process, so the all-fp32 instantiations of
mlp_fused_kernel and mlp_eval_kernel run here, in a process started with DLAMD_MLP_L1=fp32:

    python mlp_l1_child.py INPUT.npz OUTPUT.npz

INPUT holds, per case i: dims{i}, gX{i} [n, P], gdata{i} [n, 64, din], glabels{i} int32 [n, 64]
(the gradient call), eX{i} [n, P], edata{i} [rows, din] (the eval call, shared rows) and lr.
OUTPUT receives G{i} and logits{i} (row-major X), Gt{i} and logitst{i} (column-tiled X, back in
row order), T{i} (the gradient call with lr: out_mode 1) and loss{i}."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 64


def main(argv):
    if os.environ.get("DLAMD_MLP_L1", "")[:1] != "f":
        raise SystemExit("start this script with DLAMD_MLP_L1=fp32")
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch
    from distributed_learning_amd import engine
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    src, dst = argv[1], argv[2]
    d = np.load(src)
    dev = torch.device("cuda", 0)
    lr = float(d["lr"])
    out = {}

    def rows(X0):   # [n, P] view of a NaN-padded [n, ld] buffer, ld a multiple of 64
        n, P = X0.shape
        buf = torch.full((n, -(-P // 64) * 64), float("nan"), device=dev)
        buf[:, :P] = X0
        return buf[:, :P]

    i = 0
    while f"dims{i}" in d:
        dims = tuple(int(v) for v in d[f"dims{i}"])
        X0 = torch.from_numpy(d[f"gX{i}"]).to(dev)
        data = torch.from_numpy(d[f"gdata{i}"]).to(dev)
        labels = torch.from_numpy(d[f"glabels{i}"]).to(dev)
        n, P = X0.shape
        bann = BatchedANN(n, 64, *dims, device=dev, path="fused", split=False)
        X, G, T = rows(X0), rows(torch.zeros_like(X0)), rows(torch.zeros_like(X0))
        out[f"loss{i}"] = bann.gradients(X, data, labels, G).cpu().numpy()
        bann.gradients(X, data, labels, T, lr=lr)
        Xt = engine.to_tiled(X0, TILE)
        Gt = torch.full_like(Xt, float("nan"))
        bann.gradients(Xt, data, labels, Gt)
        out[f"G{i}"], out[f"T{i}"] = G.cpu().numpy(), T.cpu().numpy()
        out[f"Gt{i}"] = engine.from_tiled(Gt, P).cpu().numpy()
        E0 = torch.from_numpy(d[f"eX{i}"]).to(dev)
        edata = torch.from_numpy(d[f"edata{i}"]).to(dev)
        z = torch.full((n, edata.shape[0], dims[2]), float("nan"), device=dev)
        zt = torch.full_like(z, float("nan"))
        bann.evaluate(rows(E0), edata, None, logits=z, fused=True)
        bann.evaluate(engine.to_tiled(E0, TILE), edata, None, logits=zt, fused=True)
        out[f"logits{i}"], out[f"logitst{i}"] = z.cpu().numpy(), zt.cpu().numpy()
        i += 1
    torch.cuda.synchronize()
    np.savez(dst, **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
