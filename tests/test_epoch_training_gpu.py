"""Epoch training of c3 from a device-resident dataset: ``BatchSampler`` + ``dl_batch_gather``
inside ``MLPConsensusSGD`` (captured and replayed) against the same steps driven from Python --
the fixed-batch ``MLPConsensusSGD`` whose buffers the test refills per step by torch indexing --
bit for bit; the momentum / weight-decay optimizer against ``sgd_step`` + ``round`` applied by the
test; ``fit``'s history against direct evaluation; and the sampler's shards and shuffles.

8 agents on a random 4-regular graph, ANNModel(16, 8, 4), batch 64, 8 * 64 * 3 + 5 samples:
three full batches per agent and epoch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, B, DIMS = 8, 64, (16, 8, 4)
N_SAMPLES = N * B * 3 + 5
LR = 0.1


@pytest.fixture(scope="module")
def setup(cuda):
    from distributed_learning_amd.graph import from_edge_weights, random_regular_edges
    gen = torch.Generator(device=cuda).manual_seed(21)
    samples = torch.randn(N_SAMPLES, DIMS[0], device=cuda, generator=gen)
    targets = torch.randint(0, DIMS[2], (N_SAMPLES,), device=cuda, generator=gen,
                            dtype=torch.int32)
    test = (torch.randn(100, DIMS[0], device=cuda, generator=gen),
            torch.randint(0, DIMS[2], (100,), device=cuda, generator=gen, dtype=torch.int32))
    edges = random_regular_edges(4, N, seed=0)
    csr = from_edge_weights(edges, [0.2] * len(edges), list(range(N)))
    return dict(samples=samples, targets=targets, test=test, csr=csr, gen=gen)


def build(cuda, setup, layout, order=None, sampler=None, X0=None, **kw):
    """(engine, MLPConsensusSGD): with a sampler, or with fixed-batch buffers of its own."""
    from distributed_learning_amd import engine
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    from distributed_learning_amd.workloads import MLPConsensusSGD
    bann = BatchedANN(N, B, *DIMS, device=cuda)
    assert bann.path == "fused"
    csr = setup["csr"]
    cols = bann.P if layout == "tiled" else MLPConsensusSGD.padded_params(csr, bann.P, cuda)
    eng = engine.GossipEngine(csr, cols, device=cuda, layout=layout, order=order,
                              X=torch.nn.functional.pad(X0, (0, cols - bann.P)))
    assert eng.layout == layout
    if sampler is not None:
        return eng, MLPConsensusSGD(bann, eng, None, None, lr=LR, sampler=sampler, **kw)
    data = torch.zeros(N, B, DIMS[0], device=cuda)
    labels = torch.zeros(N, B, device=cuda, dtype=torch.int32)
    return eng, MLPConsensusSGD(bann, eng, data, labels, lr=LR, **kw)


def x0(cuda, seed=1):
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    P = BatchedANN(N, B, *DIMS, device=cuda).P
    return 0.3 * torch.randn(N, P, device=cuda,
                             generator=torch.Generator(device=cuda).manual_seed(seed))


def fill(sgd, setup, ids):
    """The parent commit's way: index the dataset from Python into the step's static buffers
    (rows in engine row order, as MLPConsensusSGD keeps them)."""
    order = sgd.eng.order
    if order is not None:
        ids = ids.index_select(0, order)
    sgd.data.copy_(setup["samples"][ids])
    sgd.labels.copy_(setup["targets"][ids])


@pytest.mark.parametrize("layout,ordered", [("rows", False), ("tiled", False), ("tiled", True)])
def test_captured_epochs_match_python_indexing(cuda, setup, layout, ordered):
    from distributed_learning_amd.workloads import BatchSampler
    order = np.random.default_rng(5).permutation(N) if ordered else None
    X0 = x0(cuda)
    sampler = BatchSampler(setup["samples"], setup["targets"], N, B, seed=4)
    assert sampler.steps == 3
    eng, sgd = build(cuda, setup, layout, order, sampler=sampler, X0=X0)
    ref_eng, ref = build(cuda, setup, layout, order, X0=X0)
    sgd.capture()
    assert sampler.cursor.item() == 0 and sgd.steps_done == 0      # capture ran nothing
    seen = []
    for s in range(7):                       # three epochs: new_epoch() at steps 0, 3, 6
        if s % 3 == 0:
            sampler.new_epoch()
        ids = sampler.batch_ids(s % 3)
        seen.append(ids.clone())
        sgd.replay()
        fill(ref, setup, ids)
        ref.step()
        assert torch.equal(eng.rows(), ref_eng.rows()), s
        assert torch.equal(sgd.agent_loss(), ref.agent_loss()), s
        assert sampler.cursor.item() == (s % 3 + 1) % 3
    assert sgd.steps_done == 7
    assert not torch.equal(eng.rows()[:, :X0.shape[1]], X0)
    # the steps of an epoch use different samples, and every agent ids of its own shard
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[0], seen[3])
    for a in range(N):
        shard = set(sampler.shards[a].tolist())
        assert all(set(ids[a].tolist()) <= shard for ids in seen)


@pytest.mark.parametrize("layout", ["rows", "tiled"])
def test_momentum_weight_decay_match_two_launches(cuda, setup, layout):
    """momentum 0.9, weight decay 5e-4 (Man_Colab cell 19): every step's X and M equal
    sgd_step(out=S) + round(src=S) applied to the same gradient with the test's own M."""
    from distributed_learning_amd.workloads import BatchSampler, sgd_step
    X0 = x0(cuda, 2)
    opt = dict(momentum=0.9, weight_decay=5e-4)
    sampler = BatchSampler(setup["samples"], setup["targets"], N, B, seed=6)
    eng, sgd = build(cuda, setup, layout, sampler=sampler, X0=X0, **opt)
    with pytest.raises(RuntimeError, match="eager step"):
        sgd.capture()
    ref_eng, ref = build(cuda, setup, layout, X0=X0)
    M = torch.zeros_like(ref_eng.X)
    S = torch.zeros_like(ref_eng.X)
    flat = (lambda t: t.view(1, -1)) if layout == "tiled" else (lambda t: t)
    for s in range(4):
        if s == 1:
            sgd.capture()
        fill(ref, setup, sampler.batch_ids(s % 3))
        if s == 0:
            sgd.step()
        else:
            sgd.replay()
        ref.gradients()
        assert torch.equal(sgd.G, ref.G), s
        sgd_step(flat(ref_eng.X), flat(ref.G), flat(M), out=flat(S), lr=LR, first=s == 0, **opt)
        ref_eng.round(src=S, deviation=True)
        assert torch.equal(eng.rows(), ref_eng.rows()), s
        assert torch.equal(sgd.M, M), s
    assert M.abs().max() > 0
    with pytest.raises(ValueError, match="emit='grad'"):
        build(cuda, setup, layout, X0=X0, emit="step", momentum=0.9)


def test_fit_history_equals_direct_evaluation(cuda, setup):
    from distributed_learning_amd.workloads import BatchSampler
    X0 = x0(cuda, 3)
    runs = []
    for captured in (True, False):
        sampler = BatchSampler(setup["samples"], setup["targets"], N, B, seed=8)
        eng, sgd = build(cuda, setup, "tiled", sampler=sampler, X0=X0)
        if captured:
            sgd.capture()
        hist = sgd.fit(epochs=2, stat_step=2, test=setup["test"])
        assert [h[0] for h in hist] == [2, 4, 6] and sgd.steps_done == 6
        assert sampler.epochs == 3                  # the constructor's and fit's two
        runs.append((hist, eng.rows().clone()))
    # the same run step by step, evaluated directly
    sampler = BatchSampler(setup["samples"], setup["targets"], N, B, seed=8)
    eng, sgd = build(cuda, setup, "tiled", sampler=sampler, X0=X0)
    direct = []
    for s in range(6):
        if s % 3 == 0:
            sampler.new_epoch()
        sgd.step()
        if (s + 1) % 2 == 0:
            loss, correct = sgd.evaluate(*setup["test"])
            direct.append((s + 1, loss.clone(), correct.clone()))
    for hist, rows in runs:
        assert torch.equal(rows, eng.rows())
        for (hs, hl, hc), (ds, dl, dc) in zip(hist, direct):
            assert hs == ds and torch.equal(hl, dl) and torch.equal(hc, dc)
            assert hl.shape == (N,) and 0 <= int(hc.min()) and int(hc.max()) <= 100
    assert not torch.equal(direct[0][1], direct[2][1])
    with pytest.raises(ValueError, match="sampler"):
        build(cuda, setup, "tiled", X0=X0)[1].fit(1)


@pytest.mark.parametrize("layout", ["rows", "tiled"])
def test_default_arguments_change_nothing(cuda, setup, layout):
    """All-default new arguments: the bits of a step are those of an object constructed
    without them."""
    from distributed_learning_amd.workloads import MLPConsensusSGD
    X0 = x0(cuda, 4)
    ids = torch.randint(0, N_SAMPLES, (N, B), device=cuda,
                        generator=torch.Generator(device=cuda).manual_seed(1))
    res = []
    for kw in (dict(), dict(sampler=None, momentum=0.0, weight_decay=0.0, dampening=0.0,
                            nesterov=False)):
        eng, sgd = build(cuda, setup, layout, X0=X0, **kw)
        assert isinstance(sgd, MLPConsensusSGD) and sgd.M is None and not sgd.optimizer
        fill(sgd, setup, ids)
        sgd.step()
        res.append((eng.rows().clone(), sgd.loss.clone(), eng.dev_sq.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # and those of the parent's step spelled out: gradients, then the fused round
    eng, sgd = build(cuda, setup, layout, X0=X0)
    fill(sgd, setup, ids)
    sgd.gradients()
    eng.round(G=sgd.G, lr=LR, deviation=True)
    assert torch.equal(eng.rows(), res[0][0]) and torch.equal(eng.dev_sq, res[0][2])


def test_sampler_shards_and_shuffles(cuda, setup):
    from distributed_learning_amd.workloads import BatchSampler
    a = BatchSampler(setup["samples"], setup["targets"], N, B, seed=11)
    sizes = [len(s) for s in a.shards]
    assert sizes == [N_SAMPLES // N] * (N - 1) + [N_SAMPLES // N + N_SAMPLES % N]
    allids = torch.cat(a.shards)
    assert sorted(allids.tolist()) == list(range(N_SAMPLES))          # disjoint, covering
    assert a.steps == min(sizes) // B == 3 and a.table.shape == (N, 3 * B)
    assert a.table.dtype == torch.int32 and a.cursor.item() == 0
    first = a.table.clone()
    ptr = a.table.data_ptr()
    for r in range(N):                        # an epoch visits no sample twice
        assert len(set(first[r].tolist())) == 3 * B
        assert set(first[r].tolist()) <= set(a.shards[r].tolist())
    a.cursor.fill_(2)
    a.new_epoch()
    assert a.table.data_ptr() == ptr and a.cursor.item() == 0         # in place, rewound
    assert not torch.equal(a.table, first)                            # a fresh order
    for s in range(3):
        assert torch.equal(a.batch_ids(s), a.table[:, s * B:(s + 1) * B].long())
    assert torch.equal(a.batch_ids(4), a.batch_ids(1))
    # the same seed draws the same shards and the same orders, another seed other ones
    b = BatchSampler(setup["samples"], setup["targets"], N, B, seed=11)
    assert all(torch.equal(x, y) for x, y in zip(a.shards, b.shards))
    assert torch.equal(b.table, first)
    b.new_epoch()
    assert torch.equal(b.table, a.table)
    c = BatchSampler(setup["samples"], setup["targets"], N, B, seed=12)
    assert not torch.equal(c.table, first)
    # next_into: one launch gathers every agent's batch and steps the cursor
    data = torch.empty(N, B, DIMS[0], device=cuda)
    labels = torch.empty(N, B, device=cuda, dtype=torch.int32)
    for s in (0, 1, 2, 0):
        ids = a.batch_ids(s)
        a.next_into(data, labels)
        assert torch.equal(data, setup["samples"][ids])
        assert torch.equal(labels, setup["targets"][ids])
    # a row order permutes the table's rows, not what an agent draws
    order = torch.tensor([3, 1, 7, 0, 2, 6, 5, 4])
    before = [b.batch_ids(s).clone() for s in range(3)]
    b.attach_order(order)
    assert torch.equal(b.table, a.table[order.to(cuda)])
    assert all(torch.equal(b.batch_ids(s), before[s]) for s in range(3))
    # given shards; a shard too small for one batch is refused
    shards = [torch.arange(r * 130, r * 130 + 130) for r in range(N)]
    d = BatchSampler(setup["samples"], setup["targets"], N, B, shards=shards)
    assert d.steps == 2 and all(set(d.table[r].tolist()) <= set(shards[r].tolist())
                                for r in range(N))
    with pytest.raises(ValueError, match="full batch"):
        BatchSampler(setup["samples"], setup["targets"], N, B,
                     shards=[torch.arange(63)] + shards[1:])
