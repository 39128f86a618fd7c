"""dl_image_batch on the GPU.  The kernel copies table entries, so every comparison is
``torch.equal`` against the header's formula written in torch on the same tensors: ``F.pad`` of
the bytes with ``fill``, the slice at (top, left), ``flip(-1)``, then ``lut[c][bytes]``.

Every dataset is about 50 samples of bytes below 255 inside one buffer whose guard regions
before and after, and whose padding between samples, hold byte 255; every table's 256 entries per
channel are distinct, and no test fills with 255: a byte read outside an image shows up as a
value the oracle does not have."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
GUARD = 4096


@pytest.fixture(scope="module")
def dev(cuda):
    return cuda


def dataset(dev, C, H, W, n=50, ld_pad=0, seed=0):
    """(samples [n, C, H, W] uint8 view, targets, lut) inside a guarded buffer."""
    g = torch.Generator(device=dev).manual_seed(seed)
    D = C * H * W
    ld = D + ld_pad
    buf = torch.full((2 * GUARD + n * ld,), 255, dtype=torch.uint8, device=dev)
    rows = buf[GUARD:GUARD + n * ld].view(n, ld)
    rows[:, :D] = torch.randint(0, 255, (n, D), device=dev, generator=g, dtype=torch.uint8)
    samples = rows[:, :D].view(n, C, H, W)
    assert samples.data_ptr() == buf.data_ptr() + GUARD and samples.stride(0) == ld
    targets = torch.randint(0, 10, (n,), device=dev, generator=g, dtype=torch.int32)
    lut = torch.stack([torch.randperm(256, device=dev, generator=g) + 256 * c
                       for c in range(C)]).float() * 0.25 - 3.0
    return samples, targets, lut.contiguous()


def draws(dev, shape, pad, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    kw = dict(device=dev, generator=g, dtype=torch.int32)
    return (torch.randint(0, 2 * pad + 1, shape, **kw) |
            (torch.randint(0, 2 * pad + 1, shape, **kw) << 8) |
            (torch.randint(0, 2, shape, **kw) << 16))


def want(samples, lut, ids, words, pad, fill=0):
    """The oracle for destination images [...]: ids and aug words of that shape (words None:
    the centre crop).  Computed on the CPU: pad, slice, flip, look up."""
    n, C, H, W = samples.shape
    ids = ids.long().clamp(0, n - 1).cpu()
    shape = tuple(ids.shape)
    if words is None:
        words = torch.full(shape, pad | (pad << 8), dtype=torch.int32)
    words = words.cpu().expand(shape).reshape(-1)
    padded = F.pad(samples.cpu(), (pad, pad, pad, pad), value=fill)
    out = torch.empty((ids.numel(), C, H, W), dtype=torch.uint8)
    for i, (sid, w) in enumerate(zip(ids.reshape(-1).tolist(), words.tolist())):
        top, left = min(w & 255, 2 * pad), min((w >> 8) & 255, 2 * pad)
        crop = padded[sid, :, top:top + H, left:left + W]
        out[i] = crop.flip(-1) if (w >> 16) & 1 else crop
    ch = torch.arange(C).view(1, C, 1, 1)
    return lut.cpu()[ch, out.long()].view(*shape, C, H, W)


def step_slice(t, batch, step):
    return t[..., step * batch:(step + 1) * batch]


# (C, H, W, pad, batch, agents, steps, ld_samples padding)
SHAPES = [(1, 1, 4, 0, 1, 1, 1, 0), (1, 28, 28, 0, 64, 3, 2, 0), (3, 32, 32, 4, 64, 2, 2, 0),
          (2, 5, 8, 3, 7, 3, 3, 16), (1, 3, 4, 6, 5, 2, 1, 0), (16, 2, 4, 1, 3, 2, 1, 0)]


@pytest.mark.parametrize("C,H,W,pad,batch,n_agents,steps,ld_pad", SHAPES)
def test_shapes_every_step(dev, C, H, W, pad, batch, n_agents, steps, ld_pad):
    from distributed_learning_amd.workloads import image_batch
    samples, targets, lut = dataset(dev, C, H, W, ld_pad=ld_pad)
    n = samples.shape[0]
    g = torch.Generator(device=dev).manual_seed(2)
    index = torch.randint(0, n, (n_agents, steps * batch), device=dev, generator=g,
                          dtype=torch.int32)
    aug = draws(dev, (n_agents, steps * batch), pad)
    for step in range(steps):
        data = torch.full((n_agents, batch, C, H, W), SENTINEL, device=dev)
        labels = torch.full((n_agents, batch), -1, device=dev, dtype=torch.int32)
        image_batch(samples, index, data, lut, aug=aug, pad=pad, targets=targets, labels=labels,
                    steps=steps, step=step)
        ids = step_slice(index, batch, step)
        d = want(samples, lut, ids, step_slice(aug, batch, step), pad)
        assert torch.equal(data.cpu(), d), (C, H, W, step)
        assert torch.equal(labels, targets[ids.long()])
    if pad > max(H, W):      # some whole outputs are the border
        assert (data[:, :, 0] == lut[0, 0]).flatten(2).all(2).any()


@pytest.mark.parametrize("C,H,W,pad", [(3, 32, 32, 4), (1, 3, 4, 2)])
def test_every_draw_of_one_sample(dev, C, H, W, pad):
    from distributed_learning_amd.workloads import image_batch
    samples, _, lut = dataset(dev, C, H, W, n=1)
    k = 2 * pad + 1
    words = torch.tensor([t | (l << 8) | (f << 16) for f in (0, 1) for t in range(k)
                          for l in range(k)], dtype=torch.int32, device=dev)
    batch = words.numel()
    assert batch == 2 * k * k
    index = torch.zeros(batch, dtype=torch.int32, device=dev)
    data = torch.full((1, batch, C, H, W), SENTINEL, device=dev)
    image_batch(samples, index, data, lut, aug=words, pad=pad)
    d = want(samples, lut, index, words, pad)
    assert torch.equal(data[0].cpu(), d)
    assert len({d[i].numpy().tobytes() for i in range(batch)}) == batch     # all different


def test_aug_handling(dev):
    from distributed_learning_amd.workloads import image_batch
    C, H, W, pad, batch, n_agents, steps = 3, 8, 12, 2, 6, 3, 2
    samples, _, lut = dataset(dev, C, H, W)
    g = torch.Generator(device=dev).manual_seed(5)
    index = torch.randint(0, 50, (n_agents, steps * batch), device=dev, generator=g,
                          dtype=torch.int32)
    run = lambda aug, step=1: image_batch(                                   # noqa: E731
        samples, index, torch.full((n_agents, batch, C, H, W), SENTINEL, device=dev), lut,
        aug=aug, pad=pad, steps=steps, step=step)
    ids = step_slice(index, batch, 1)
    # aug = None is the explicit centre words: the test transform
    centre = torch.full((n_agents, steps * batch), pad | (pad << 8), dtype=torch.int32,
                        device=dev)
    none = run(None)
    assert torch.equal(none, run(centre))
    assert torch.equal(none.cpu(), want(samples, lut, ids, None, pad))
    assert torch.equal(none.cpu(), samples_lut(samples, lut)[ids.long().cpu()])
    # one list of draws shared by all agents (s_aug = 0)
    shared = draws(dev, (steps * batch,), pad, seed=7)
    got = run(shared)
    assert torch.equal(got.cpu(), want(samples, lut, ids, step_slice(shared, batch, 1), pad))
    # bits 17 and up are ignored
    aug = draws(dev, (n_agents, steps * batch), pad, seed=8)
    high = torch.randint(0, 1 << 14, aug.shape, device=dev, generator=g, dtype=torch.int32) << 17
    assert torch.equal(run(aug), run(aug | high))
    assert torch.equal(run(aug), run(aug | -(1 << 17)))
    # top and left above 2 * pad are clamped to it
    over = aug.clone()
    over[:, ::2] |= 0xFF
    over[:, 1::3] |= 0xC800
    clamped = over.clone()
    clamped[:, ::2] = (clamped[:, ::2] & ~0xFF) | 2 * pad
    clamped[:, 1::3] = (clamped[:, 1::3] & ~0xFF00) | (2 * pad << 8)
    got = run(over)
    assert torch.equal(got, run(clamped))
    assert torch.equal(got.cpu(), want(samples, lut, ids, step_slice(over, batch, 1), pad))


def samples_lut(samples, lut):
    """lut[c][bytes] of the whole dataset, on the CPU."""
    C = samples.shape[1]
    return lut.cpu()[torch.arange(C).view(1, C, 1, 1), samples.cpu().long()]


@pytest.mark.parametrize("C,H,W,pad", [(3, 32, 32, 4), (2, 5, 8, 3)])
def test_edges(dev, C, H, W, pad):
    """A fill other than 0; the first and the last sample (next to the guard regions) at the
    extreme offsets; ids out of range, clamped; repeated ids."""
    from distributed_learning_amd.workloads import image_batch
    samples, targets, lut = dataset(dev, C, H, W, ld_pad=0 if C == 3 else 16)
    n = samples.shape[0]
    corners = [t | (l << 8) | (f << 16) for f in (0, 1) for t in (0, 2 * pad)
               for l in (0, 2 * pad)]
    ids = [0] * 8 + [n - 1] * 8 + [-1, n, n + 1000, -2**31, 2**31 - 1, 7, 7, 7]
    index = torch.tensor([ids, ids[::-1]], dtype=torch.int32, device=dev)
    words = torch.tensor([corners * 3, corners * 3], dtype=torch.int32, device=dev)
    batch = len(ids)
    for fill in (37, 0, 254):
        data = torch.full((2, batch, C, H, W), SENTINEL, device=dev)
        labels = torch.full((2, batch), -1, device=dev, dtype=torch.int32)
        image_batch(samples, index, data, lut, aug=words, pad=pad, fill=fill, targets=targets,
                    labels=labels)
        assert torch.equal(data.cpu(), want(samples, lut, index, words, pad, fill)), fill
        assert torch.equal(labels, targets[index.long().clamp(0, n - 1)])
    # the border is lut[c][fill]: the top left pixel of an image cropped at (0, 0)
    assert torch.equal(data[0, 0, :, 0, 0], lut[:, 254])


@pytest.mark.parametrize("C,H,W,pad,batch", [(1, 28, 28, 0, 64), (2, 5, 8, 3, 7)])
def test_padding_survives(dev, C, H, W, pad, batch):
    """s_data > batch * C*H*W and an oversized labels buffer: what lies between the agents'
    blocks keeps its sentinel."""
    from distributed_learning_amd.workloads import image_batch
    n_agents, steps, D = 3, 2, C * H * W
    samples, targets, lut = dataset(dev, C, H, W)
    g = torch.Generator(device=dev).manual_seed(3)
    index = torch.randint(0, 50, (n_agents, steps * batch), device=dev, generator=g,
                          dtype=torch.int32)
    aug = draws(dev, index.shape, pad)
    s_data, s_lab = batch * D + 8, batch + 3
    dbuf = torch.full((n_agents, s_data), SENTINEL, device=dev)
    lbuf = torch.full((n_agents, s_lab), -5, device=dev, dtype=torch.int32)
    data = dbuf[:, :batch * D].view(n_agents, batch, C, H, W)
    assert data.stride(0) == s_data and data.data_ptr() == dbuf.data_ptr()
    image_batch(samples, index, data, lut, aug=aug, pad=pad, targets=targets,
                labels=lbuf[:, :batch], steps=steps, step=1)
    ids = step_slice(index, batch, 1)
    assert torch.equal(data.cpu(), want(samples, lut, ids, step_slice(aug, batch, 1), pad))
    assert torch.equal(lbuf[:, :batch], targets[ids.long()])
    assert (dbuf[:, batch * D:] == SENTINEL).all() and (lbuf[:, batch:] == -5).all()
    # the flat [N, batch, C*H*W] spelling of data is the same call
    flat = torch.full((n_agents, batch, D), SENTINEL, device=dev)
    image_batch(samples, index, flat, lut, aug=aug, pad=pad, steps=steps, step=1)
    assert torch.equal(flat.view_as(data), data)


def test_no_labels(dev):
    from distributed_learning_amd.workloads import image_batch
    C, H, W, pad = 2, 5, 8, 3
    samples, targets, lut = dataset(dev, C, H, W)
    index = torch.randint(0, 50, (3, 10), device=dev, dtype=torch.int32,
                          generator=torch.Generator(device=dev).manual_seed(4))
    aug = draws(dev, index.shape, pad)
    d = want(samples, lut, step_slice(index, 5, 1), step_slice(aug, 5, 1), pad)
    data = torch.full((3, 5, C, H, W), SENTINEL, device=dev)
    image_batch(samples, index, data, lut, aug=aug, pad=pad, steps=2, step=1)   # targets NULL too
    assert torch.equal(data.cpu(), d)
    data.fill_(SENTINEL)
    image_batch(samples, index, data, lut, aug=aug, pad=pad, targets=targets, steps=2, step=1)
    assert torch.equal(data.cpu(), d)
    with pytest.raises(ValueError, match="labels need targets"):
        image_batch(samples, index, data, lut, pad=pad, steps=2,
                    labels=torch.zeros(3, 5, device=dev, dtype=torch.int32))
    with pytest.raises(ValueError, match="uint8"):
        image_batch(samples.float(), index, data, lut, steps=2)
    with pytest.raises(ValueError, match="pad must lie"):
        image_batch(samples, index, data, lut, pad=128, steps=2)


def test_host_step_is_taken_mod_steps(dev):
    from distributed_learning_amd.workloads import image_batch
    C, H, W, pad, batch, n_agents, steps = 2, 5, 8, 3, 7, 2, 3
    samples, _, lut = dataset(dev, C, H, W)
    index = torch.randint(0, 50, (n_agents, steps * batch), device=dev, dtype=torch.int32,
                          generator=torch.Generator(device=dev).manual_seed(6))
    aug = draws(dev, index.shape, pad)
    d = [want(samples, lut, step_slice(index, batch, s), step_slice(aug, batch, s), pad)
         for s in range(steps)]
    for step in (0, 2, 3, 7, 3 * 1000 + 1, -1, -3, -2**31):
        data = torch.full((n_agents, batch, C, H, W), SENTINEL, device=dev)
        image_batch(samples, index, data, lut, aug=aug, pad=pad, steps=steps, step=step)
        assert torch.equal(data.cpu(), d[step % steps]), step
    with pytest.raises(ValueError, match="advance needs a cursor"):
        image_batch(samples, index, data, lut, aug=aug, pad=pad, steps=steps, advance=True)


@pytest.fixture(scope="module")
def stepping(dev):
    """One CIFAR-shaped problem and its oracle per step, shared by the cursor tests."""
    C, H, W, pad, batch, n_agents, steps = 3, 32, 32, 4, 16, 3, 2
    samples, targets, lut = dataset(dev, C, H, W)
    index = torch.randint(0, 50, (n_agents, steps * batch), device=dev, dtype=torch.int32,
                          generator=torch.Generator(device=dev).manual_seed(9))
    aug = draws(dev, index.shape, pad)
    d = [want(samples, lut, step_slice(index, batch, s), step_slice(aug, batch, s), pad).to(dev)
         for s in range(steps)]
    lab = [targets[step_slice(index, batch, s).long()] for s in range(steps)]
    return dict(samples=samples, targets=targets, lut=lut, index=index, aug=aug, d=d, lab=lab,
                pad=pad, steps=steps, shape=(n_agents, batch, C, H, W))


def test_device_cursor_walks_the_epoch(dev, stepping):
    from distributed_learning_amd.workloads import image_batch
    p, steps = stepping, stepping["steps"]
    cursor = torch.zeros(1, device=dev, dtype=torch.int32)
    data = torch.empty(p["shape"], device=dev)
    labels = torch.empty(p["shape"][:2], device=dev, dtype=torch.int32)

    def call(advance=True, labels=None):
        data.fill_(SENTINEL)
        image_batch(p["samples"], p["index"], data, p["lut"], aug=p["aug"], pad=p["pad"],
                    targets=p["targets"], labels=labels, steps=steps, cursor=cursor,
                    advance=advance)
    for s in list(range(steps)) * 2 + [0]:                   # 2 * steps + 1 calls
        call(labels=labels)
        assert torch.equal(data, p["d"][s]) and torch.equal(labels, p["lab"][s]), s
    assert cursor.item() == 1 % steps
    call(advance=False)                    # without advance the cursor is read and left alone
    assert torch.equal(data, p["d"][1 % steps]) and cursor.item() == 1 % steps
    cursor.fill_(steps - 1)                # the last step wraps to 0
    call()
    assert torch.equal(data, p["d"][steps - 1]) and cursor.item() == 0
    cursor.fill_(-1)                       # a cursor outside [0, steps) is taken mod steps
    call()
    assert torch.equal(data, p["d"][steps - 1]) and cursor.item() == 0


def test_replayed_graph_equals_eager_calls(dev, stepping):
    from distributed_learning_amd.workloads import image_batch
    p, steps = stepping, stepping["steps"]
    cursor = torch.zeros(1, device=dev, dtype=torch.int32)
    data = torch.full(p["shape"], SENTINEL, device=dev)
    labels = torch.full(p["shape"][:2], -1, device=dev, dtype=torch.int32)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        image_batch(p["samples"], p["index"], data, p["lut"], aug=p["aug"], pad=p["pad"],
                    targets=p["targets"], labels=labels, steps=steps, cursor=cursor,
                    advance=True)
    assert cursor.item() == 0 and (data == SENTINEL).all()      # capture ran nothing
    for s in list(range(steps)) * 2 + [0]:                       # 2 * steps + 1 replays
        g.replay()
        assert torch.equal(data, p["d"][s]) and torch.equal(labels, p["lab"][s]), s
    assert cursor.item() == 1 % steps


def test_dataset_past_4_gib(dev):
    """Row bases are 64-bit: the last samples of a 4 GiB + 16 KiB dataset (never initialised but
    for its first and last 8 samples) come back; a 32-bit byte offset would wrap to the first."""
    from distributed_learning_amd.workloads import image_batch
    n, C, H, W, pad, batch = 2**21 + 8, 2, 32, 32, 4, 16
    if torch.cuda.mem_get_info(dev)[0] < 6 * 2**30:
        pytest.skip("less than 6 GiB of free device memory")
    try:
        samples = torch.empty((n, C, H, W), device=dev, dtype=torch.uint8)
    except RuntimeError as e:          # torch.cuda.OutOfMemoryError is one
        pytest.skip(f"cannot allocate the 4 GiB dataset: {str(e)[:80]}")
    g = torch.Generator(device=dev).manual_seed(3)
    ends = torch.randint(0, 255, (16, C, H, W), device=dev, generator=g, dtype=torch.uint8)
    samples[:8], samples[-8:] = ends[:8], ends[8:]
    lut = (torch.randperm(512, device=dev, generator=g).view(2, 256).float() - 100.0)
    sel = torch.randperm(16)
    ids = torch.cat([torch.arange(8), torch.arange(n - 8, n)])[sel]
    index = ids.to(dev, torch.int32)
    aug = draws(dev, (batch,), pad)
    data = torch.full((1, batch, C, H, W), SENTINEL, device=dev)
    image_batch(samples, index, data, lut, aug=aug, pad=pad)
    # the oracle on the 16 initialised samples alone, in the same order
    d = want(ends[sel.to(dev)], lut, torch.arange(16), aug, pad)
    assert torch.equal(data[0].cpu(), d)
    assert (ids >= 8).sum() == 8 and not torch.equal(ends[:8], ends[8:])
    del samples
