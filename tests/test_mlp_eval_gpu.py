"""dl_mlp_eval (BatchedANN.evaluate, MLPConsensusSGD.evaluate): every agent's test loss, correct
count and logits in one launch, against the project's ANNModel run in fp64 on the CPU and, bit
for bit, against the loss of the gradient kernel whose forward it shares.
The logits' tight bound (fp32 rounding level, per agent) lives in tests/test_mlp_x6_gpu.py."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MARGIN = 1e-4     # fp64 top-2 logit margin below which a row's argmax may go either way


@functools.lru_cache(maxsize=None)
def case(n, rows, dims, shared, seed=0):
    """Models (torch.manual_seed(seed)), data and labels (Generator().manual_seed(1)) and the
    fp64 forward of every agent on the CPU, computed once per shape and never modified."""
    from distributed_learning_amd.networks import ANNModel
    din, dh, dout = dims
    torch.manual_seed(seed)
    models = [ANNModel(din, dh, dout) for _ in range(n)]
    X0 = torch.stack([torch.cat([p.data.reshape(-1) for p in m.parameters()]) for m in models])
    gen = torch.Generator().manual_seed(1)
    shape = (rows,) if shared else (n, rows)
    data = torch.randn(*shape, din, generator=gen)
    labels = torch.randint(0, dout, shape, generator=gen, dtype=torch.int32)
    with torch.no_grad():
        z = torch.stack([copy.deepcopy(m).double()(data.double() if shared else data[a].double())
                         for a, m in enumerate(models)])            # [n, rows, dout] fp64
    top2 = z.topk(2, dim=2).values
    return dict(X0=X0, data=data, labels=labels, z=z, sure=(top2[..., 0] - top2[..., 1]) >= MARGIN,
                argmax=z.argmax(2))


def ref_stats(c, labels):
    """fp64 mean cross-entropy [n] and, per agent, the correct count over the sure rows and the
    number of unsure rows."""
    z = c["z"]
    lab = labels.long().expand(z.shape[0], z.shape[1])
    loss = (torch.logsumexp(z, 2) - z.gather(2, lab.unsqueeze(2)).squeeze(2)).mean(1)
    hit = (c["argmax"] == lab) & c["sure"]
    return loss.numpy(), hit.sum(1).numpy(), (~c["sure"]).sum(1).numpy()


def padded_rows(X0, dev, fill=0.0):
    """[n, P] view of a [n, ld] buffer, ld a multiple of 64 (16-byte aligned rows, as the
    engine keeps them)."""
    n, P = X0.shape
    buf = torch.full((n, -(-P // 64) * 64), fill, device=dev)
    buf[:, :P] = X0.to(dev)
    return buf[:, :P]


def check_against_fp64(c, labels, loss, correct, logits):
    z = c["z"].numpy()
    if logits is not None:
        np.testing.assert_allclose(logits.cpu().numpy(), z, rtol=1e-4,
                                   atol=1e-5 * np.abs(z).max())
    want_loss, want_hit, unsure = ref_stats(c, labels)
    assert unsure.sum() <= 0.01 * z.shape[0] * z.shape[1]
    got_loss, got_hit = loss.cpu().numpy(), correct.cpu().numpy()
    for a in range(z.shape[0]):
        assert got_loss[a] == pytest.approx(want_loss[a], rel=1e-5), a
        assert want_hit[a] <= got_hit[a] <= want_hit[a] + unsure[a], a


@pytest.mark.parametrize("layout", ["rows", "tiled"])
def test_same_bits_as_the_training_loss(cuda, layout):
    """A full block's loss is dl_mlp_grad's loss of those 64 rows bit for bit, and two blocks
    reduce as the header states: (float)(((double)l0 + (double)l1) * 64 / 128)."""
    from distributed_learning_amd import engine
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    n, dims = 3, (52, 40, 7)
    c = case(n, 128, dims, False)
    bann = BatchedANN(n, 64, *dims, device=cuda, path="fused")
    data, labels = c["data"].to(cuda), c["labels"].to(cuda)
    if layout == "rows":
        X = padded_rows(c["X0"], cuda)
        G = padded_rows(c["X0"], cuda)                   # overwritten: the same row geometry
    else:
        X = engine.to_tiled(c["X0"].to(cuda), 64)
        G = torch.empty_like(X)
    halves = []
    for h in range(2):
        d, lab = data[:, 64 * h:64 * h + 64].contiguous(), labels[:, 64 * h:64 * h + 64].contiguous()
        halves.append(bann.gradients(X, d, lab, G).clone())
        loss, correct = bann.evaluate(X, d, lab)
        assert torch.equal(loss, halves[h]), h
    loss, _ = bann.evaluate(X, data, labels)
    l0, l1 = (t.cpu().numpy() for t in halves)
    want = ((l0.astype(np.float64) + l1.astype(np.float64)) * 64 / 128).astype(np.float32)
    assert np.array_equal(loss.cpu().numpy().view(np.uint32), want.view(np.uint32))


CASES = [(3, 200, (52, 40, 7), True), (2, 136, (784, 150, 10), True),
         (3, 64, (16, 152, 16), False), (5, 129, (20, 24, 5), False),
         (3, 1, (52, 40, 7), True), (3, 63, (52, 40, 7), True)]


@pytest.mark.parametrize("n,rows,dims,shared", CASES)
def test_against_the_fp64_forward(cuda, n, rows, dims, shared):
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    c = case(n, rows, dims, shared)
    bann = BatchedANN(n, 32, *dims, device=cuda)        # any training batch
    X = padded_rows(c["X0"], cuda)
    data, labels = c["data"].to(cuda), c["labels"].to(cuda)
    logits = torch.full((n, rows, dims[2]), float("nan"), device=cuda)
    loss, correct = bann.evaluate(X, data, labels, logits=logits)
    assert bann.eval_ws is not None                     # the kernel, not the layered forward
    check_against_fp64(c, c["labels"], loss, correct, logits)
    # every agent labelled by its own fp64 argmax: all rows correct
    own = c["argmax"].to(torch.int32)
    _, correct = bann.evaluate(X, data, own.to(cuda))
    unsure = (~c["sure"]).sum(1)
    got = correct.cpu()
    assert torch.all(got <= rows) and torch.all(got >= rows - unsure)
    if unsure.sum() == 0:
        assert torch.all(got == rows)


def test_gradient_fixture_loss(cuda, golden):
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    d = golden("mlp_grad_small.npz")
    din, dh, dout = (int(v) for v in d["dims"])
    n, b = d["data"].shape[:2]
    bann = BatchedANN(n, b, din, dh, dout, device=cuda)
    loss, correct = bann.evaluate(padded_rows(torch.from_numpy(d["X"]), cuda),
                                  torch.from_numpy(d["data"]).to(cuda),
                                  torch.from_numpy(d["labels"]).to(cuda))
    for a in range(n):
        assert loss[a].item() == pytest.approx(float(d["loss"][a]), rel=1e-5)
    assert torch.all((correct >= 0) & (correct <= b))


def test_results_do_not_depend_on_the_grid(cuda):
    from distributed_learning_amd import engine
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    n, rows, dims = 3, 200, (52, 40, 7)
    c = case(n, rows, dims, True)
    bann = BatchedANN(n, 64, *dims, device=cuda)
    data, labels = c["data"].to(cuda), c["labels"].to(cuda)
    outs = []
    for X in (padded_rows(c["X0"], cuda), engine.to_tiled(c["X0"].to(cuda), 64)):
        for splits in (1, 3, 0, 0, 1000):
            logits = torch.full((n, rows, dims[2]), float("nan"), device=cuda)
            loss, correct = bann.evaluate(X, data, labels, logits=logits, row_splits=splits)
            outs.append((loss.clone(), correct.clone(), logits))
    for loss, correct, logits in outs[1:]:
        assert torch.equal(loss, outs[0][0]) and torch.equal(correct, outs[0][1])
        assert torch.equal(logits, outs[0][2])
    assert torch.isfinite(outs[0][2]).all()


@pytest.mark.parametrize("rows", [200, 129])
def test_containment(cuda, rows):
    """NaN in X's padding columns changes nothing; nothing is written outside [rows][dout] of
    the logits; logits alone need no labels."""
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    n, dims = 3, (52, 40, 7)
    dout = dims[2]
    c = case(n, rows, dims, True)
    bann = BatchedANN(n, 64, *dims, device=cuda)
    data, labels = c["data"].to(cuda), c["labels"].to(cuda)
    loss0, correct0 = (t.clone() for t in bann.evaluate(padded_rows(c["X0"], cuda), data, labels))
    Xn = padded_rows(c["X0"], cuda, fill=float("nan"))
    assert Xn.stride(0) > Xn.shape[1]
    buf = torch.full((n, rows + 5, dout + 3), float("nan"), device=cuda)
    loss, correct = bann.evaluate(Xn, data, labels, logits=buf[:, :rows, :dout])
    assert torch.equal(loss, loss0) and torch.equal(correct, correct0)
    assert torch.isfinite(buf[:, :rows, :dout]).all()
    assert torch.isnan(buf[:, rows:]).all() and torch.isnan(buf[:, :, dout:]).all()
    buf2 = torch.full_like(buf, float("nan"))
    assert bann.evaluate(Xn, data, None, logits=buf2[:, :rows, :dout]) == (None, None)
    assert torch.equal(buf2[:, :rows, :dout], buf[:, :rows, :dout])
    assert torch.isnan(buf2[:, rows:]).all() and torch.isnan(buf2[:, :, dout:]).all()
    check_against_fp64(c, c["labels"], loss, correct, buf[:, :rows, :dout])


def test_layered_fallback(cuda):
    """Shapes the kernel refuses (input_dim % 4 != 0) run the dl_bgemm forward, and so does
    evaluate(fused=False) on any row-major call."""
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    n, rows, dims = 4, 100, (50, 40, 7)
    for shared in (True, False):
        c = case(n, rows, dims, shared)
        bann = BatchedANN(n, 64, *dims, device=cuda)
        logits = torch.full((n, rows, dims[2]), float("nan"), device=cuda)
        loss, correct = bann.evaluate(padded_rows(c["X0"], cuda), c["data"].to(cuda),
                                      c["labels"].to(cuda), logits=logits)
        assert bann.eval_ws is None                     # no kernel workspace: the layered path
        check_against_fp64(c, c["labels"], loss, correct, logits)
        with pytest.raises(ValueError):
            bann.evaluate(padded_rows(c["X0"], cuda), c["data"].to(cuda), c["labels"].to(cuda),
                          fused=True)
    # fused=False: the layered forward on a shape the kernel covers (fused=None and True: the
    # kernel); the tiled layout has no layered forward
    n, rows, dims = 3, 200, (52, 40, 7)
    c = case(n, rows, dims, True)
    bann = BatchedANN(n, 64, *dims, device=cuda)
    X, data, labels = padded_rows(c["X0"], cuda), c["data"].to(cuda), c["labels"].to(cuda)
    logits = torch.full((n, rows, dims[2]), float("nan"), device=cuda)
    loss, correct = bann.evaluate(X, data, labels, logits=logits, fused=False)
    assert bann.eval_ws is None
    check_against_fp64(c, c["labels"], loss, correct, logits)
    kl = torch.full_like(logits, float("nan"))
    bann.evaluate(X, data, labels, logits=kl, fused=True)
    assert bann.eval_ws is not None
    kn = torch.full_like(logits, float("nan"))
    bann.evaluate(X, data, labels, logits=kn)
    assert torch.equal(kn, kl)
    with pytest.raises(ValueError):
        from distributed_learning_amd import engine
        bann.evaluate(engine.to_tiled(c["X0"].to(cuda), 64), data, labels, fused=False)


@pytest.mark.parametrize("layout", ["rows", "tiled"])
def test_consensus_workload_evaluate(cuda, layout):
    """MLPConsensusSGD.evaluate reads eng.X in its layout (zero padding columns included), returns
    agent order under an engine row order, and replays from a hipGraph with the eager bits."""
    from distributed_learning_amd import engine
    from distributed_learning_amd.graph import from_edge_weights, random_regular_edges
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    from distributed_learning_amd.workloads import MLPConsensusSGD
    n, rows, dims = 16, 129, (52, 40, 7)
    gen = torch.Generator().manual_seed(1)
    bann = BatchedANN(n, 64, *dims, device=cuda)
    P = bann.P
    X0 = (0.3 * torch.randn(n, P, generator=gen)).to(cuda)
    train = torch.randn(n, 64, dims[0], generator=gen).to(cuda)
    train_lab = torch.randint(0, dims[2], (n, 64), generator=gen, dtype=torch.int32).to(cuda)
    test = torch.randn(rows, dims[0], generator=gen).to(cuda)
    test_lab = torch.randint(0, dims[2], (rows,), generator=gen, dtype=torch.int32).to(cuda)
    own = torch.randn(n, rows, dims[0], generator=gen).to(cuda)
    own_lab = torch.randint(0, dims[2], (n, rows), generator=gen, dtype=torch.int32).to(cuda)
    edges = random_regular_edges(4, n, seed=0)
    csr = from_edge_weights(edges, [0.2] * len(edges), list(range(n)))
    cols = P if layout == "tiled" else MLPConsensusSGD.padded_params(csr, P, cuda)
    perm = np.random.default_rng(3).permutation(n)
    res = {}
    for name, order in (("agents", None), ("perm", perm)):
        eng = engine.GossipEngine(csr, cols, device=cuda, layout=layout, order=order,
                                  X=torch.nn.functional.pad(X0, (0, cols - P)))
        assert eng.layout == layout
        sgd = MLPConsensusSGD(bann, eng, train, train_lab, lr=0.1)
        sgd.step()
        direct = BatchedANN(n, 64, *dims, device=cuda)
        Xrows = padded_rows(eng.rows()[:, :P], cuda)
        out = []
        for d, lab in ((test, test_lab), (own, own_lab)):
            want = [t.clone() for t in direct.evaluate(Xrows, d, lab)]
            wl = torch.full((n, rows, dims[2]), float("nan"), device=cuda)
            direct.evaluate(Xrows, d, None, logits=wl)
            gl = torch.full_like(wl, float("nan"))
            got = [t.clone() for t in sgd.evaluate(d, lab, logits=gl)]
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            assert torch.equal(gl, wl)
            out.append(want)
        res[name] = out
        # captured and replayed: the eager bits
        eager = [t.clone() for t in sgd.evaluate(test, test_lab)]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cap = sgd.evaluate(test, test_lab)
        for t in cap:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap[0], eager[0]) and torch.equal(cap[1], eager[1])
    for a, b in zip(res["agents"], res["perm"]):        # the row order changes nothing
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
