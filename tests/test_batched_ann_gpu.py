"""Batched per-agent MLP gradients (config c3) against plain PyTorch fp32 autograd, one
ANNModel per agent (reference networks/ann_model.py + torch.nn.CrossEntropyLoss).
The fused path's tight bound (fp32 rounding level, per parameter block, against float64) lives in
tests/test_mlp_x6_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _flat_grads(m):
    return torch.cat([p.grad.reshape(-1) for p in m.parameters()])


@pytest.mark.parametrize("n,b,dims,path", [(4, 64, (784, 150, 10), "layers"),
                                           (4, 64, (784, 150, 10), "fused"),
                                           (5, 64, (52, 40, 7), "fused"),
                                           (3, 64, (16, 152, 16), "fused"),
                                           (7, 33, (50, 40, 7), "auto"),
                                           (3, 5, (20, 15, 3), "auto"),
                                           # batch > 64: plain bias epilogue + dl_xent_grad, and
                                           # the > 64-row tile selector on the batch-row GEMMs
                                           (2, 80, (20, 24, 5), "auto")])
def test_gradients_match_autograd(cuda, n, b, dims, path):
    from distributed_learning_amd.networks import ANNModel
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    din, dh, dout = dims
    torch.manual_seed(0)
    models = [ANNModel(din, dh, dout).to(cuda) for _ in range(n)]
    X0 = torch.stack([torch.cat([p.data.reshape(-1) for p in m.parameters()]) for m in models])
    P = X0.shape[1]
    ld = -(-P // 64) * 64          # padded rows: 16-byte aligned, as the engine keeps them
    X = torch.zeros(n, ld, device=cuda)[:, :P]
    X.copy_(X0)
    data = torch.randn(n, b, din, device=cuda)
    labels = torch.randint(0, dout, (n, b), device=cuda, dtype=torch.int32)
    bann = BatchedANN(n, b, din, dh, dout, device=cuda, path=path)
    assert bann.path == (path if path != "auto" else "layers")
    assert bann.P == X.shape[1]
    Gbuf = torch.full((n, ld), float("nan"), device=cuda)
    G = Gbuf[:, :P]
    loss = bann.gradients(X, data, labels, G).clone()
    torch.cuda.synchronize()
    for a, m in enumerate(models):
        m.zero_grad()
        ref_loss = torch.nn.functional.cross_entropy(m(data[a]), labels[a].long())
        ref_loss.backward()
        ref = _flat_grads(m)
        assert torch.isfinite(G[a]).all()
        scale = ref.abs().max().item()
        np.testing.assert_allclose(G[a].cpu().numpy(), ref.cpu().numpy(), rtol=1e-4,
                                   atol=1e-5 * scale)
        assert loss[a].item() == pytest.approx(ref_loss.item(), rel=1e-5)
    assert torch.isnan(Gbuf[:, P:]).all()       # nothing written past the parameter columns


@pytest.mark.parametrize("layout", ["rows", "tiled"])
@pytest.mark.parametrize("n,dims", [(4, (784, 150, 10)), (5, (52, 40, 7)), (3, (16, 152, 16))])
def test_step_output_is_the_local_sgd_step(cuda, n, dims, layout):
    """dl_mlp_args.out_mode 1: the kernel writes T = X - lr G instead of G -- bit for bit
    fl(x - fl(lr g)) of the same kernel's gradient launch (what dl_mix_round's fused step
    computes), in both resident layouts, and nothing outside the parameter columns."""
    from distributed_learning_amd import engine
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    din, dh, dout = dims
    gen = torch.Generator(device=cuda).manual_seed(21)
    bann = BatchedANN(n, 64, din, dh, dout, device=cuda, path="fused")
    P, lr = bann.P, 0.07
    X0 = 0.1 * torch.randn(n, P, device=cuda, generator=gen)
    data = torch.randn(n, 64, din, device=cuda, generator=gen)
    labels = torch.randint(0, dout, (n, 64), device=cuda, generator=gen, dtype=torch.int32)
    if layout == "rows":
        ld = -(-P // 64) * 64
        X = torch.zeros(n, ld, device=cuda)
        X[:, :P] = X0
        G, T = (torch.full((n, ld), float("nan"), device=cuda) for _ in range(2))
        bann.gradients(X[:, :P], data, labels, G[:, :P])
        bann.gradients(X[:, :P], data, labels, T[:, :P], lr=lr)
        torch.cuda.synchronize()
        g, t = G[:, :P], T[:, :P]
        assert torch.isnan(T[:, P:]).all()
    else:
        X = engine.to_tiled(X0, 8)
        G, T = (torch.full_like(X, float("nan")) for _ in range(2))
        bann.gradients(X, data, labels, G)
        bann.gradients(X, data, labels, T, lr=lr)
        torch.cuda.synchronize()
        g, t = engine.from_tiled(G, P), engine.from_tiled(T, P)
        assert torch.isnan(T.reshape(-1, n, 8).permute(1, 0, 2).reshape(n, -1)[:, P:]).all()
    assert torch.isfinite(g).all()
    want = X0 - g * lr               # two fp32 roundings: fl(x - fl(lr g))
    assert torch.equal(t, want)
    with pytest.raises(ValueError):
        BatchedANN(n, 64, din, dh, dout, device=cuda, path="layers").gradients(
            X0, data, labels, torch.empty_like(X0), lr=lr)


def test_consensus_sgd_round_with_batched_grads(cuda):
    """One c3 round: G from the batched kernels, then the fused local step + mix; equals the
    per-agent autograd step followed by the oracle mix (to fp32 GEMM rounding)."""
    from distributed_learning_amd import engine
    from distributed_learning_amd.graph import from_edge_weights, random_regular_edges
    from distributed_learning_amd.networks import ANNModel
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    from oracle import cref
    n, b = 16, 32
    torch.manual_seed(1)
    models = [ANNModel(64, 32, 10).to(cuda) for _ in range(n)]
    X = torch.stack([torch.cat([p.data.reshape(-1) for p in m.parameters()]) for m in models])
    data = torch.randn(n, b, 64, device=cuda)
    labels = torch.randint(0, 10, (n, b), device=cuda, dtype=torch.int32)
    edges = random_regular_edges(4, n, seed=0)
    csr = from_edge_weights(edges, [0.2] * len(edges), list(range(n)))
    bann = BatchedANN(n, b, 64, 32, 10, device=cuda)
    eng = engine.GossipEngine(csr, bann.P, device=cuda, X=X, layout="rows")
    G = torch.empty_like(X)
    bann.gradients(eng.X, data, labels, G)
    eng.round(G=G, lr=0.1)
    torch.cuda.synchronize()
    grads = []
    for a, m in enumerate(models):
        m.zero_grad()
        torch.nn.functional.cross_entropy(m(data[a]), labels[a].long()).backward()
        grads.append(_flat_grads(m))
    want = cref.mix_round(X.cpu().numpy(), csr.rowptr, csr.col, csr.w,
                          G=torch.stack(grads).cpu().numpy(), lr=0.1)
    np.testing.assert_allclose(eng.rows().cpu().numpy(), want, rtol=1e-5, atol=1e-6)


def test_mlp_consensus_graph_replay_matches_eager(cuda):
    """c3 steps recorded as hipGraphs (two ping-pong graphs) give the same bits as eager steps,
    for an odd and an even number of steps."""
    from distributed_learning_amd import engine
    from distributed_learning_amd.graph import from_edge_weights, random_regular_edges
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    from distributed_learning_amd.workloads import MLPConsensusSGD
    n, b = 16, 32
    gen = torch.Generator(device=cuda).manual_seed(5)
    bann = BatchedANN(n, b, 64, 32, 10, device=cuda)
    X0 = 0.1 * torch.randn(n, bann.P, device=cuda, generator=gen)
    data = torch.randn(n, b, 64, device=cuda, generator=gen)
    labels = torch.randint(0, 10, (n, b), device=cuda, generator=gen, dtype=torch.int32)
    edges = random_regular_edges(4, n, seed=0)
    csr = from_edge_weights(edges, [0.2] * len(edges), list(range(n)))
    runs = {}
    for mode in ("eager", "graph"):
        eng = engine.GossipEngine(csr, bann.P, device=cuda, X=X0, layout="rows")
        sgd = MLPConsensusSGD(bann, eng, data, labels, lr=0.1)
        out = []
        if mode == "graph":
            sgd.capture()
            assert torch.equal(eng.X, X0)          # capture ran nothing
        for k in (3, 2):
            if mode == "graph":
                sgd.replay(k)
            else:
                for _ in range(k):
                    sgd.step()
            torch.cuda.synchronize()
            out.append((eng.X.clone(), eng.dev_sq.clone(), sgd.loss.clone()))
        runs[mode] = out
    for (xe, de, le), (xg, dg, lg) in zip(runs["eager"], runs["graph"]):
        assert torch.equal(xe, xg) and torch.equal(de, dg) and torch.equal(le, lg)
    assert not torch.equal(runs["eager"][0][0], X0)


def test_mlp_consensus_zero_padding_is_exact(cuda):
    """Zero padding columns up to a whole mix tile (no ragged tail launch) leave the real
    columns bit-identical to the unpadded round; the deviation sums the same terms (plus exact
    zeros) grouped by a different launch split, so it agrees to fp32 rounding."""
    from distributed_learning_amd import engine
    from distributed_learning_amd.graph import from_edge_weights, random_regular_edges
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    from distributed_learning_amd.workloads import MLPConsensusSGD
    n, b = 32, 16
    gen = torch.Generator(device=cuda).manual_seed(9)
    bann = BatchedANN(n, b, 40, 24, 10, device=cuda)
    P = bann.P
    X0 = 0.2 * torch.randn(n, P, device=cuda, generator=gen)
    data = torch.randn(n, b, 40, device=cuda, generator=gen)
    labels = torch.randint(0, 10, (n, b), device=cuda, generator=gen, dtype=torch.int32)
    edges = random_regular_edges(4, n, seed=2)
    csr = from_edge_weights(edges, [0.2] * len(edges), list(range(n)))
    P_pad = MLPConsensusSGD.padded_params(csr, P, cuda)
    assert P_pad > P
    res = []
    for cols in (P, P_pad):
        eng = engine.GossipEngine(csr, cols, device=cuda,
                                  X=torch.nn.functional.pad(X0, (0, cols - P)), layout="rows")
        sgd = MLPConsensusSGD(bann, eng, data, labels, lr=0.2)
        for _ in range(3):
            sgd.step()
        torch.cuda.synchronize()
        assert torch.all(eng.X[:, P:] == 0)
        res.append((eng.X[:, :P].clone(), eng.dev_sq.clone()))
    assert torch.equal(res[0][0], res[1][0])
    torch.testing.assert_close(res[0][1], res[1][1], rtol=1e-5, atol=0)


def test_mlp_consensus_tiled_layout_matches_rows(cuda):
    """c3 with X and G in the engine's column-tiled layout (the fused kernel addresses the tiles,
    the round streams whole HBM blocks) gives the same parameters, bit for bit, as the
    row-major layout; the deviation agrees to fp32 rounding (different reduction split)."""
    from distributed_learning_amd import engine
    from distributed_learning_amd.graph import from_edge_weights, random_regular_edges
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    from distributed_learning_amd.workloads import MLPConsensusSGD
    n, b = 48, 64
    gen = torch.Generator(device=cuda).manual_seed(11)
    bann = BatchedANN(n, b, 100, 60, 10, device=cuda)
    assert bann.path == "fused"
    P = bann.P
    X0 = 0.1 * torch.randn(n, P, device=cuda, generator=gen)
    data = torch.randn(n, b, 100, device=cuda, generator=gen)
    labels = torch.randint(0, 10, (n, b), device=cuda, generator=gen, dtype=torch.int32)
    edges = random_regular_edges(4, n, seed=4)
    csr = from_edge_weights(edges, [0.2] * len(edges), list(range(n)))
    res = {}
    for layout in ("rows", "tiled"):
        cols = P if layout == "tiled" else MLPConsensusSGD.padded_params(csr, P, cuda)
        X = X0 if layout == "tiled" else torch.nn.functional.pad(X0, (0, cols - P))
        eng = engine.GossipEngine(csr, cols, device=cuda, X=X, layout=layout)
        assert eng.layout == layout
        sgd = MLPConsensusSGD(bann, eng, data, labels, lr=0.1)
        for _ in range(3):
            sgd.step()
        torch.cuda.synchronize()
        res[layout] = (eng.rows()[:, :P].clone(), eng.dev_sq.clone(), sgd.loss.clone())
    assert torch.equal(res["rows"][0], res["tiled"][0])
    assert torch.equal(res["rows"][2], res["tiled"][2])
    torch.testing.assert_close(res["rows"][1], res["tiled"][1], rtol=1e-5, atol=0)


@pytest.mark.parametrize("layout", ["rows", "tiled"])
def test_mlp_consensus_step_emission_matches_gradient_emission(cuda, layout):
    """MLPConsensusSGD(emit="step") -- the kernel writes X - lr G, the round mixes it -- gives the
    parameters, losses and deviation of emit="grad" (the kernel writes G, the fused round forms
    X - lr G) bit for bit, eager and under hipGraph replay."""
    from distributed_learning_amd import engine
    from distributed_learning_amd.graph import from_edge_weights, random_regular_edges
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    from distributed_learning_amd.workloads import MLPConsensusSGD
    n, b = 40, 64
    gen = torch.Generator(device=cuda).manual_seed(13)
    bann = BatchedANN(n, b, 96, 50, 10, device=cuda)
    P = bann.P
    X0 = 0.1 * torch.randn(n, P, device=cuda, generator=gen)
    data = torch.randn(n, b, 96, device=cuda, generator=gen)
    labels = torch.randint(0, 10, (n, b), device=cuda, generator=gen, dtype=torch.int32)
    edges = random_regular_edges(4, n, seed=6)
    csr = from_edge_weights(edges, [0.2] * len(edges), list(range(n)))
    cols = P if layout == "tiled" else MLPConsensusSGD.padded_params(csr, P, cuda)
    res = {}
    for emit in ("grad", "step", "step-graph"):
        eng = engine.GossipEngine(csr, cols, device=cuda,
                                  X=torch.nn.functional.pad(X0, (0, cols - P)), layout=layout)
        sgd = MLPConsensusSGD(bann, eng, data, labels, lr=0.1, emit=emit.split("-")[0])
        assert sgd.emit == emit.split("-")[0]
        if emit == "step-graph":
            sgd.capture()
            sgd.replay(3)
        else:
            for _ in range(3):
                sgd.step()
        torch.cuda.synchronize()
        res[emit] = (eng.rows().clone(), eng.dev_sq.clone(), sgd.loss.clone())
    for emit in ("step", "step-graph"):
        for a, b_ in zip(res["grad"], res[emit]):
            assert torch.equal(a, b_), emit
    assert MLPConsensusSGD(bann, engine.GossipEngine(csr, cols, device=cuda, layout=layout),
                           data, labels, lr=0.1).emit == "grad"


@pytest.mark.parametrize("layout", ["rows", "tiled"])
def test_mlp_consensus_follows_the_engine_row_order(cuda, layout):
    """An engine row order (``GossipEngine(order=...)``; "auto" picks one on plan-path-5 graphs)
    stores agent order[s] in row s.  MLPConsensusSGD permutes the per-agent batches with it, so
    every agent still trains on its own data: parameters (``eng.rows()``), per-agent losses and
    deviations equal those of the unpermuted engine bit for bit."""
    from distributed_learning_amd import engine
    from distributed_learning_amd.graph import from_edge_weights, random_regular_edges
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    from distributed_learning_amd.workloads import MLPConsensusSGD
    n, b = 48, 64
    gen = torch.Generator(device=cuda).manual_seed(17)
    bann = BatchedANN(n, b, 100, 60, 10, device=cuda)
    P = bann.P
    X0 = 0.1 * torch.randn(n, P, device=cuda, generator=gen)
    data = torch.randn(n, b, 100, device=cuda, generator=gen)
    labels = torch.randint(0, 10, (n, b), device=cuda, generator=gen, dtype=torch.int32)
    edges = random_regular_edges(4, n, seed=8)
    csr = from_edge_weights(edges, [0.2] * len(edges), list(range(n)))
    cols = P if layout == "tiled" else MLPConsensusSGD.padded_params(csr, P, cuda)
    perm = np.random.default_rng(3).permutation(n)
    res = {}
    for name, order in (("agents", None), ("perm", perm)):
        eng = engine.GossipEngine(csr, cols, device=cuda, layout=layout, order=order,
                                  X=torch.nn.functional.pad(X0, (0, cols - P)))
        sgd = MLPConsensusSGD(bann, eng, data, labels, lr=0.1)
        for _ in range(3):
            sgd.step()
        torch.cuda.synchronize()
        res[name] = (eng.rows().clone(), sgd.agent_loss().clone(), eng.agent_dev_sq().clone())
    assert torch.equal(res["agents"][0], res["perm"][0])
    assert torch.equal(res["agents"][1], res["perm"][1])
    torch.testing.assert_close(res["agents"][2], res["perm"][2], rtol=1e-5, atol=0)


@pytest.mark.parametrize("layout", ["rows", "tiled"])
@pytest.mark.parametrize("n,dims", [(256, (784, 150, 10)), (16, (784, 150, 10)),
                                    (5, (52, 40, 7)), (3, (16, 152, 16)), (24, (100, 60, 10)),
                                    (1, (784, 150, 10)), (7, (416, 96, 16))])
def test_split_gradients_equal_the_one_launch_kernel(cuda, n, dims, layout):
    """dl_mlp_grad with a workspace runs two launches (everything up to dZ1, then dW1 over x's
    column tiles on two workgroups per agent); every split, product and summation order is the
    one-launch kernel's, so gradients and losses are bit-identical, and nothing is written past
    the parameter columns."""
    from distributed_learning_amd import engine
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    din, dh, dout = dims
    gen = torch.Generator(device=cuda).manual_seed(29)
    one = BatchedANN(n, 64, din, dh, dout, device=cuda, path="fused", split=False)
    three = BatchedANN(n, 64, din, dh, dout, device=cuda, path="fused", split=True)
    assert one.ws is None and three.ws is not None
    P = one.P
    X0 = 0.1 * torch.randn(n, P, device=cuda, generator=gen)
    data = torch.randn(n, 64, din, device=cuda, generator=gen)
    labels = torch.randint(0, dout, (n, 64), device=cuda, generator=gen, dtype=torch.int32)
    out = []
    for bann in (one, three):
        if layout == "rows":
            ld = -(-P // 64) * 64
            X = torch.zeros(n, ld, device=cuda)
            X[:, :P] = X0
            G = torch.full((n, ld), float("nan"), device=cuda)
            loss = bann.gradients(X[:, :P], data, labels, G[:, :P]).clone()
            torch.cuda.synchronize()
            assert torch.isnan(G[:, P:]).all()
            g = G[:, :P]
        else:
            X = engine.to_tiled(X0, 8)
            G = torch.full_like(X, float("nan"))
            loss = bann.gradients(X, data, labels, G).clone()
            torch.cuda.synchronize()
            g = engine.from_tiled(G, P)
        assert torch.isfinite(g).all()
        out.append((g.clone(), loss))
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
    # the workspace is reused step after step: a second call gives the same bits again
    if layout == "rows":
        G2 = torch.full((n, ld), float("nan"), device=cuda)
        three.gradients(X[:, :P], data, labels, G2[:, :P])
        torch.cuda.synchronize()
        assert torch.equal(G2[:, :P], out[0][0])
