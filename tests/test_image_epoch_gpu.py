"""Epoch training from a ``uint8`` image dataset: ``ImageBatchSampler`` + ``dl_image_batch``.

The sampler's index table against ``BatchSampler``'s, its draws, and ``next_into`` against the
header's formula in torch (pad, slice, flip, table lookup); c3 through ``MLPConsensusSGD`` bit
for bit against the fp32 ``BatchSampler`` run on the converted dataset; c5 through
``WRNConsensusSGD(sampler=...)`` and ``fit`` bit for bit against a second instance stepped by
hand on the oracle's batches, eager and captured; and the default path unchanged."""
import os

import pytest
import torch
import torch.nn.functional as F

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")   # small test shapes: skip MIOpen's search

pytestmark = pytest.mark.gpu

MNIST = ((0.1307,), (0.3081,))
CIFAR = ((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))


def images(cuda, n, C, H, W, seed):
    g = torch.Generator(device=cuda).manual_seed(seed)
    return (torch.randint(0, 256, (n, C, H, W), device=cuda, generator=g, dtype=torch.uint8),
            torch.randint(0, 10, (n,), device=cuda, generator=g, dtype=torch.int32))


def want(samples, lut, ids, draws, pad, fill=0):
    """The oracle: fp32 [N, batch, C, H, W] for ids and (top, left, flip) of shape [N, batch]:
    ``F.pad`` of the bytes, the slice, ``flip(-1)``, then ``lut[c][bytes]``; on the device."""
    n, C, H, W = samples.shape
    top, left, flip = (d.reshape(-1).tolist() for d in draws)
    padded = F.pad(samples, (pad, pad, pad, pad), value=fill)
    out = torch.empty((ids.numel(), C, H, W), dtype=torch.uint8, device=samples.device)
    for i, sid in enumerate(ids.reshape(-1).tolist()):
        crop = padded[sid, :, top[i]:top[i] + H, left[i]:left[i] + W]
        out[i] = crop.flip(-1) if flip[i] else crop
    ch = torch.arange(C, device=samples.device).view(1, C, 1, 1)
    return lut[ch, out.long()].view(*ids.shape, C, H, W)


def test_lut_is_totensor_normalize(cuda):
    """The table is torchvision's pixel: ToTensor's byte / 255, then Normalize's sub, div, all
    fp32 -- spelled out here on every byte value."""
    from distributed_learning_amd.workloads import ImageBatchSampler
    img, tg = images(cuda, 16, 3, 4, 4, 0)
    s = ImageBatchSampler(img, tg, 2, 4, *CIFAR)
    assert s.lut.shape == (3, 256) and s.lut.dtype == torch.float32
    byte = torch.arange(256, dtype=torch.uint8).view(1, 256, 1).expand(3, 256, 1)
    x = byte.to(torch.float32).div(255)                     # ToTensor on a [3, 256, 1] image
    mean = torch.as_tensor(CIFAR[0], dtype=torch.float32).view(-1, 1, 1)
    std = torch.as_tensor(CIFAR[1], dtype=torch.float32).view(-1, 1, 1)
    assert torch.equal(s.lut.cpu(), x.sub_(mean).div_(std).view(3, 256))   # Normalize
    assert s.dim == 48 and s.shape == (3, 4, 4) and s.samples.dtype == torch.uint8


def test_sampler_tables_draws_and_batches(cuda):
    from distributed_learning_amd.workloads import BatchSampler, ImageBatchSampler
    N, B, C, H, W, pad = 3, 5, 3, 8, 12, 2
    img, tg = images(cuda, 50, C, H, W, 1)
    a = ImageBatchSampler(img, tg, N, B, *CIFAR, pad=pad, flip=True, seed=11)
    ref = BatchSampler(img.float(), tg, N, B, seed=11)
    assert a.steps == ref.steps == 3 and (a.n_agents, a.batch, a.dim) == (N, B, C * H * W)
    assert a.aug.shape == a.table.shape and a.aug.dtype == torch.int32
    assert all(torch.equal(x, y) for x, y in zip(a.shards, ref.shards))
    b = ImageBatchSampler(img, tg, N, B, *CIFAR, pad=pad, flip=True, seed=11)
    c = ImageBatchSampler(img, tg, N, B, *CIFAR, pad=pad, flip=True, seed=12)
    seen, seen_table = [], a.table.clone()      # the first epoch's ids
    ptrs = (a.table.data_ptr(), a.aug.data_ptr())
    for epoch in range(3):
        # the index table is BatchSampler's; the draws are reproducible for one seed
        assert torch.equal(a.table, ref.table) and torch.equal(a.table, b.table), epoch
        assert torch.equal(a.aug, b.aug) and not torch.equal(a.aug, c.aug)
        top, left, flip = (torch.cat([a.aug_draws(s)[k] for s in range(a.steps)], 1)
                           for k in range(3))
        assert torch.equal(top | (left << 8) | (flip << 16), a.aug.long())
        assert 0 <= int(top.min()) and int(top.max()) <= 2 * pad
        assert 0 <= int(left.min()) and int(left.max()) <= 2 * pad
        assert set(flip.flatten().tolist()) == {0, 1}
        assert len(set(top.flatten().tolist())) > 1 and len(set(left.flatten().tolist())) > 1
        seen.append(a.aug.clone())
        a.cursor.fill_(2)
        for s in (a, b, c, ref):
            s.new_epoch()
        assert (a.table.data_ptr(), a.aug.data_ptr()) == ptrs and a.cursor.item() == 0
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert a.epochs == 4
    # without flip the flip bit stays clear; without pad the words are zero
    d = ImageBatchSampler(img, tg, N, B, *CIFAR, pad=pad, seed=11)
    assert not (d.aug >> 16).any() and (d.aug & 0xFFFF).any() and torch.equal(d.table, seen_table)
    assert not ImageBatchSampler(img, tg, N, B, *CIFAR, seed=11).aug.any()
    # next_into is the oracle on batch_ids and aug_draws; a row order permutes the tables' rows,
    # not what an agent draws
    order = torch.tensor([2, 0, 1])
    before = [(b.batch_ids(s).clone(), [t.clone() for t in b.aug_draws(s)]) for s in range(3)]
    b.attach_order(order)
    assert torch.equal(b.table, a.table[order.to(cuda)])
    assert torch.equal(b.aug, a.aug[order.to(cuda)])
    data = torch.empty(N, B, C, H, W, device=cuda)
    flat = torch.empty(N, B, C * H * W, device=cuda)
    labels = torch.empty(N, B, device=cuda, dtype=torch.int32)
    for s in (0, 1, 2, 0):
        ids, dr = a.batch_ids(s), a.aug_draws(s)
        assert torch.equal(ids, before[s][0])
        assert all(torch.equal(x, y) for x, y in zip(b.aug_draws(s), before[s][1]))
        d = want(a.samples, a.lut, ids, dr, pad)
        a.next_into(data, labels)
        assert torch.equal(data, d) and torch.equal(labels, tg[ids])
        b.next_into(flat, labels)                    # rows in table order, flat data
        assert torch.equal(flat.view_as(data), d[order.to(cuda)])
        assert torch.equal(labels, tg[ids][order.to(cuda)])
    assert a.cursor.item() == 1
    # the test transform through the same table
    ev = a.eval_transform(img[:7].cpu())
    ch = torch.arange(C, device=cuda).view(1, C, 1, 1)
    assert ev.shape == (7, C, H, W) and torch.equal(ev, a.lut[ch, img[:7].long()])
    with pytest.raises(ValueError, match="multiple of 4"):
        ImageBatchSampler(img[..., :10], tg, N, B, *CIFAR)
    with pytest.raises(ValueError, match="uint8"):
        ImageBatchSampler(img.float(), tg, N, B, *CIFAR)


# ---- c3: MLPConsensusSGD on 1 x 28 x 28 bytes against the fp32 BatchSampler run ----
N3, B3, DIMS3 = 4, 64, (784, 16, 10)


def build_c3(cuda, csr, sampler, X0):
    from distributed_learning_amd import engine
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    from distributed_learning_amd.workloads import MLPConsensusSGD
    bann = BatchedANN(N3, B3, *DIMS3, device=cuda)
    assert bann.path == "fused"
    eng = engine.GossipEngine(csr, bann.P, device=cuda, layout="tiled", X=X0)
    return eng, MLPConsensusSGD(bann, eng, None, None, lr=0.1, sampler=sampler)


@pytest.mark.parametrize("captured", [False, True])
def test_c3_epochs_equal_the_fp32_sampler(cuda, captured):
    from distributed_learning_amd.graph import from_edge_weights
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    from distributed_learning_amd.workloads import BatchSampler, ImageBatchSampler
    edges = [(i, (i + 1) % N3) for i in range(N3)]
    csr = from_edge_weights(edges, [0.25] * len(edges), list(range(N3)))
    img, tg = images(cuda, N3 * B3 * 2 + 5, 1, 28, 28, 2)
    u8 = ImageBatchSampler(img, tg, N3, B3, *MNIST, seed=4)
    f32 = BatchSampler(u8.eval_transform(img), tg, N3, B3, seed=4)     # lut[0][bytes]
    assert u8.steps == f32.steps == 2 and u8.dim == f32.dim == 784
    P = BatchedANN(N3, B3, *DIMS3, device=cuda).P
    X0 = 0.1 * torch.randn(N3, P, device=cuda,
                           generator=torch.Generator(device=cuda).manual_seed(1))
    runs = [build_c3(cuda, csr, s, X0) for s in (u8, f32)]
    for eng, sgd in runs:
        if captured:
            sgd.capture()
        sgd.fit(epochs=2)
        assert sgd.steps_done == 4 and sgd.sampler.epochs == 3
    (e0, s0), (e1, s1) = runs
    assert torch.equal(u8.table, f32.table)
    assert torch.equal(s0.data, s1.data) and torch.equal(s0.labels, s1.labels)
    assert torch.equal(e0.rows(), e1.rows()) and torch.equal(s0.agent_loss(), s1.agent_loss())
    assert not torch.equal(e0.rows(), X0)


# ---- c5: WRNConsensusSGD(sampler=...) ----
@pytest.fixture
def deterministic_convs():
    """MIOpen's default conv/BN solvers are not run-to-run deterministic (split-K atomics): two
    eager runs differ by ~1e-8 after one step.  Deterministic solvers make runs comparable bit
    for bit."""
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


def ring4():
    from distributed_learning_amd.graph import best_constant_weight, uniform_weights
    edges = [(i, (i + 1) % 4) for i in range(4)]
    return uniform_weights(edges, best_constant_weight(edges))


def test_c5_fit_equals_steps_on_the_oracle_batches(cuda, deterministic_convs):
    from distributed_learning_amd.workloads import ImageBatchSampler, WRNConsensusSGD
    N, B, pad = 4, 4, 4
    img, tg = images(cuda, 48, 3, 32, 32, 3)
    kw = dict(depth=10, widen=1, lr=0.05, device=cuda, seed=1)
    sam = [ImageBatchSampler(img, tg, N, B, *CIFAR, pad=pad, flip=True, seed=5) for _ in range(3)]
    assert sam[0].steps == 3
    eager = WRNConsensusSGD(ring4(), B, sampler=sam[0], **kw)
    assert eager.data.shape == (N, B, 3, 32, 32) and eager.data.dtype == torch.float32
    assert eager.labels.dtype == torch.int64 and eager.labels32.dtype == torch.int32
    eager.fit(2)
    # a second instance on static buffers, stepped by hand on the oracle's batches
    hand = WRNConsensusSGD(ring4(), B, data=torch.zeros(N, B, 3, 32, 32, device=cuda),
                           labels=torch.zeros(N, B, dtype=torch.int64, device=cuda), **kw)
    s = sam[1]
    for _ in range(2):
        s.new_epoch()
        for step in range(s.steps):
            ids = s.batch_ids(step)
            hand.data.copy_(want(s.samples, s.lut, ids, s.aug_draws(step), pad))
            hand.labels.copy_(tg[ids])
            hand.step()
    torch.cuda.synchronize()
    assert eager.steps_done == hand.steps_done == 6
    assert torch.equal(eager.data, hand.data) and torch.equal(eager.labels, hand.labels)
    assert torch.equal(eager.params(), hand.params())
    assert torch.equal(eager.M, hand.M) and torch.equal(eager.loss, hand.loss)
    # captured after one eager step: the replays walk the epochs by themselves
    cap = WRNConsensusSGD(ring4(), B, sampler=sam[2], **kw)
    with pytest.raises(RuntimeError, match="eager step"):
        cap.capture()
    sam[2].new_epoch()
    cap.step()
    cap.capture()
    assert sam[2].cursor.item() == 1 and cap.steps_done == 1       # capture ran nothing
    cap.replay(2)
    cap.fit(1)                                                      # new_epoch + 3 replays
    torch.cuda.synchronize()
    assert cap.steps_done == 6 and sam[2].epochs == sam[0].epochs == 3
    assert torch.equal(cap.params(), eager.params())
    assert torch.equal(cap.M, eager.M) and torch.equal(cap.loss, eager.loss)
    with pytest.raises(ValueError, match="pass None"):
        WRNConsensusSGD(ring4(), B, sampler=sam[0], data=hand.data, labels=hand.labels, **kw)


def test_c5_defaults_change_nothing(cuda, deterministic_convs):
    """Without a sampler the workload is what it was: two instances, one constructed with the
    new argument spelled out, hold the same parameters after 2 steps on the same fixed batch."""
    from distributed_learning_amd.workloads import WRNConsensusSGD
    kw = dict(depth=10, widen=1, lr=0.05, device=cuda, seed=1)
    a = WRNConsensusSGD(ring4(), 4, **kw)
    b = WRNConsensusSGD(ring4(), 4, sampler=None, **kw)
    assert b.sampler is None and b.labels32 is None
    assert torch.equal(a.data, b.data) and torch.equal(a.labels, b.labels)
    assert a.data.shape == (4, 4, 3, 32, 32) and a.labels.dtype == torch.int64
    for _ in range(2):
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.params(), b.params()) and torch.equal(a.M, b.M)
    assert torch.equal(a.loss, b.loss) and a.steps_done == b.steps_done == 2
    with pytest.raises(ValueError, match="sampler"):
        a.fit(1)
