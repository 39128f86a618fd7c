"""Reference workloads driven through the drop-in API (config c1 of BASELINE.json).

Titanic consensus GD (notebooks/Titanic Consensus GD test.ipynb, cells 12-14): every agent holds
a contiguous shard of the training set, takes a local GD step on the L2-regularised logistic
loss with step ``alpha * (it + 1) ** -0.5`` and then runs one asyncio consensus round weighted
by its shard size.  Data preparation (cells 2-4) lives with the caller; the tests feed the
preprocessed arrays committed under tests/golden/.
"""
import asyncio

import numpy as np

from .networks.logreg_model_titanic import LogRegTitanic
from .utils import consensus_asyncio as ca


def split_data(X, y, tokens):
    """``split_data`` (notebook cell 12): contiguous shards in ``tokens`` order."""
    tmpX, tmpy = X.copy(), y.copy()
    result = {}
    num = len(tokens)
    for i in range(num):
        ln = len(tmpX) // (num - i)
        result[tokens[i]] = (tmpX[:ln], tmpy[:ln])
        tmpX, tmpy = tmpX[ln:], tmpy[ln:]
    return result


async def _learning_instance(X, y, agent, iterations, alpha, tau, schedule):
    model = LogRegTitanic(X.shape[1], lr=alpha, tau=tau)
    w = np.zeros(X.shape[1])
    for it in range(iterations):
        grad = model.gradient(X, y, w)
        step = alpha * np.power(it + 1, -0.5) if schedule == "sqrt" else alpha
        w = w - step * grad
        w = await agent.run_round(w, X.shape[0])
    return w


async def consensus_gd(topology, X, y, iterations, alpha=1e-1, tau=1e-4, convergence_eps=1e-10,
                       schedule="sqrt", device=None, consensus="reference"):
    """``run`` of the notebook (cell 14) without plots: the learning tasks are created first and
    the master's ``serve`` after them, as the notebook does.  ``consensus`` picks the façade's
    schedule ("reference": the reference's own message interleaving, each agent step on the
    device; "synchronous": one Jacobi launch per round).  Returns {token: final w}."""
    shutdown = asyncio.Queue()
    net = ca.ConsensusNetwork(topology, shutdown, device=device, schedule=consensus)
    agents = [ca.ConsensusAgent(t, convergence_eps=convergence_eps) for t in net.tokens]
    for a in agents:
        net.register_agent(a)
    shards = split_data(X, y, net.tokens)
    tasks = [asyncio.create_task(_learning_instance(*shards[a.token], a, iterations, alpha, tau,
                                                    schedule)) for a in agents]
    serve = asyncio.create_task(net.serve())
    res = await asyncio.gather(*tasks)
    await shutdown.put(ca.SHUTDOWN)
    await serve
    return {a.token: w for a, w in zip(agents, res)}


class ConsensusGDRun:
    """``consensus_gd`` with every agent and every iteration in ONE launch (dl_consensus_gd):
    the same shards (``split_data`` in ``ConsensusNetwork.tokens`` order), local steps and
    consensus rounds (weighted by shard size, ``convergence_eps`` one-sided test), fp64 on the
    device with no host round trip per iteration.  The constructor makes everything resident
    (shards, adjacency, step sizes, zero weights); ``launch()`` is stream-ordered; ``result()``
    copies back ({token: final w}, Jacobi iterations per round).
    ``edge_weight``: mix with a uniform per-edge weight w (x' = x(1 - w deg) + w sum_j x_j, the
    TCP agent's update with a fast-averaging weight, consensus_tcp/agent.py:204-207) instead of
    the asyncio network's Perron eps 0.95 / max degree (consensus_asyncio.py:78-86).  The FDLA
    optimum is such a uniform weight on edge-transitive graphs (ring, torus)."""

    def __init__(self, topology, X, y, iterations, alpha=1e-1, tau=1e-4, convergence_eps=1e-10,
                 schedule="sqrt", device=None, max_iter=10_000_000, edge_weight=None):
        import torch

        from . import _lib
        from .graph import asyncio_adjacency, perron_eps
        self._torch, self._lib = torch, _lib
        self.dev = torch.device(device) if device is not None else torch.device(
            "cuda", torch.cuda.current_device())
        self.tokens, rp, cl = asyncio_adjacency(topology)
        shards = split_data(X, y, self.tokens)
        Xs = np.concatenate([shards[t][0] for t in self.tokens]).astype(np.float64)
        ys = np.concatenate([shards[t][1] for t in self.tokens]).astype(np.float64)
        sizes = [shards[t][0].shape[0] for t in self.tokens]
        sp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        steps = np.asarray([alpha * np.power(it + 1, -0.5) if schedule == "sqrt" else alpha
                            for it in range(iterations)], np.float64)
        self.rows, self.iterations = int(Xs.shape[0]), int(iterations)
        F = X.shape[1]
        self.t = {k: torch.as_tensor(v, device=self.dev) for k, v in
                  dict(X=Xs, y=ys, sp=sp, rp=rp.astype(np.int32), cl=cl.astype(np.int32),
                       steps=steps if iterations else np.zeros(1),
                       w=np.zeros((len(self.tokens), F))).items()}
        self.iters = torch.zeros(max(iterations, 1), dtype=torch.int32, device=self.dev)
        t = self.t
        self.args = _lib.DlConsensusGdArgs(
            _lib.ptr(t["X"]), _lib.ptr(t["y"]), _lib.ptr(t["sp"]), len(self.tokens), F,
            _lib.ptr(t["rp"]), _lib.ptr(t["cl"]),
            float(perron_eps(topology, self.tokens) if edge_weight is None else edge_weight),
            float(convergence_eps), sum(sizes) / len(sizes), float(tau), _lib.ptr(t["steps"]),
            self.iterations, int(max_iter), _lib.ptr(t["w"]), _lib.ptr(self.iters))

    def launch(self, reset=True):
        """All iterations from zero weights (reset) on the current stream."""
        import ctypes
        if reset:
            self.t["w"].zero_()
        with self._torch.cuda.device(self.dev):
            self._lib.check(self._lib.load().dl_consensus_gd(
                ctypes.byref(self.args), self.rows, self._lib.stream_handle(self.dev)),
                "dl_consensus_gd")

    def result(self):
        wf = self.t["w"].cpu().numpy()
        return ({tok: wf[i] for i, tok in enumerate(self.tokens)},
                self.iters[:self.iterations].cpu().numpy())


def consensus_gd_device(topology, X, y, iterations, alpha=1e-1, tau=1e-4, convergence_eps=1e-10,
                        schedule="sqrt", device=None, max_iter=10_000_000, edge_weight=None):
    """One-launch ``consensus_gd`` (ConsensusGDRun).  Returns ({token: final w}, Jacobi
    iterations per round)."""
    run = ConsensusGDRun(topology, X, y, iterations, alpha, tau, convergence_eps, schedule,
                         device, max_iter, edge_weight)
    run.launch()
    return run.result()


def accuracy(w, X, y):
    m = LogRegTitanic(X.shape[1])
    m.W = w
    return m.calc_accuracy(X, y)


def batch_gather(samples, index, data, targets=None, labels=None, steps=1, cursor=None, step=0,
                 advance=False, dim=None):
    """``dl_batch_gather``: with s = (cursor[0] if cursor is given, else step) mod steps,
    ``data[a, b, :dim] = samples[index[a, s * batch + b], :dim]`` and, with labels,
    ``labels[a, b] = targets[that id]``; ``advance`` then steps the cursor to (s + 1) mod steps.

    samples: fp32 [n, >= dim] rows (row stride = ld_samples; dim defaults to the row length);
    targets: int32 [n]; index: int32 [N, steps * batch], or [steps * batch] shared by all agents;
    data: fp32 [N, batch, dim] whose agent stride may exceed batch * dim; labels: int32
    [N, batch] whose agent stride may exceed batch; cursor: device int32[1].  Ids outside
    [0, n) are clamped.  Stream-ordered, no host synchronisation, capturable in a hipGraph."""
    import ctypes

    import torch

    from . import _lib
    dim = int(samples.shape[1] if dim is None else dim)
    if samples.dim() != 2 or samples.dtype != torch.float32 or samples.stride(1) != 1 or \
            dim > samples.shape[1]:
        raise ValueError("samples must be fp32 [n, >= dim] with contiguous rows")
    if data.dim() != 3 or data.dtype != torch.float32 or data.shape[2] != dim or \
            data.stride(2) != 1 or data.stride(1) != dim:
        raise ValueError(f"data must be fp32 [N, batch, {dim}] with contiguous batches")
    n_agents, batch = int(data.shape[0]), int(data.shape[1])
    if index.dtype != torch.int32 or index.dim() not in (1, 2) or index.stride(-1) != 1 or \
            index.shape[-1] != int(steps) * batch or \
            (index.dim() == 2 and index.shape[0] != n_agents):
        raise ValueError(f"index must be int32 [{n_agents}, steps * batch] or [steps * batch]")
    if targets is not None and (targets.dtype != torch.int32 or targets.dim() != 1 or
                                targets.shape[0] != samples.shape[0] or
                                not targets.is_contiguous()):
        raise ValueError("targets must be contiguous int32 [n]")
    if labels is not None and (labels.dtype != torch.int32 or labels.stride(1) != 1 or
                               tuple(labels.shape) != (n_agents, batch)):
        raise ValueError(f"labels must be int32 [{n_agents}, {batch}]")
    if cursor is not None and (cursor.dtype != torch.int32 or cursor.numel() != 1):
        raise ValueError("cursor must be one int32")
    for t in (index, targets, labels, cursor, data):
        if t is not None and t.device != samples.device:
            raise ValueError("every operand must live on the samples' device")
    args = _lib.DlBatchGatherArgs(
        _lib.ptr(samples), samples.stride(0), _lib.ptr(targets), samples.shape[0], dim,
        _lib.ptr(index), index.stride(0) if index.dim() == 2 and n_agents > 1 else 0, n_agents,
        batch, int(steps), _lib.ptr(cursor), int(step), int(bool(advance)), _lib.ptr(data),
        data.stride(0), _lib.ptr(labels), labels.stride(0) if labels is not None else 0)
    with torch.cuda.device(samples.device):
        _lib.check(_lib.load().dl_batch_gather(ctypes.byref(args),
                                               _lib.stream_handle(samples.device)),
                   "dl_batch_gather")
    return data


def image_batch(samples, index, data, lut, aug=None, pad=0, fill=0, targets=None, labels=None,
                steps=1, cursor=None, step=0, advance=False):
    """``dl_image_batch``: with s = (cursor[0] if cursor is given, else step) mod steps and
    id = index[a, s * batch + b], ``data[a, b, c, y, x] = lut[c, P(c, y + top - pad,
    (W - 1 - x if flip else x) + left - pad)]`` where P is sample id's byte inside the image and
    ``fill`` outside, (top, left, flip) = bits 0-7, 8-15 and 16 of ``aug[a, s * batch + b]``
    (aug None: the centre crop, no flip) -- torchvision's pad, crop, flip, ``ToTensor`` +
    ``Normalize`` with the last two as the table -- and, with labels, ``labels[a, b] =
    targets[id]``; ``advance`` then steps the cursor to (s + 1) mod steps.

    samples: uint8 [n, C, H, W] planar images (sample stride >= C*H*W, W % 4 == 0); lut: fp32
    [C, 256]; targets: int32 [n]; index, aug: int32 [N, steps * batch], or [steps * batch] shared
    by all agents; data: fp32 [N, batch, C, H, W] or [N, batch, C*H*W] whose agent stride may
    exceed one batch; labels: int32 [N, batch] whose agent stride may exceed batch; cursor:
    device int32[1].  Ids outside [0, n) and offsets above 2 * pad are clamped.  Stream-ordered,
    no host synchronisation, capturable in a hipGraph."""
    import ctypes

    import torch

    from . import _lib
    if samples.dim() != 4 or samples.dtype != torch.uint8:
        raise ValueError("samples must be uint8 [n, C, H, W]")
    n, C, H, W = (int(v) for v in samples.shape)
    dim = C * H * W
    if n < 1 or dim < 1 or samples[0].stride() != (H * W, W, 1) or \
            (n > 1 and samples.stride(0) < dim):
        raise ValueError("samples must be uint8 [n, C, H, W] with contiguous planar images")
    if lut.dtype != torch.float32 or tuple(lut.shape) != (C, 256) or not lut.is_contiguous():
        raise ValueError(f"lut must be contiguous fp32 [{C}, 256]")
    if data.dtype != torch.float32 or data.dim() not in (3, 5) or \
            tuple(data.shape[2:]) not in ((dim,), (C, H, W)) or not data[0].is_contiguous():
        raise ValueError(f"data must be fp32 [N, batch, {C}, {H}, {W}] or [N, batch, {dim}] "
                         "with contiguous batches")
    n_agents, batch = int(data.shape[0]), int(data.shape[1])
    for name, t in (("index", index), ("aug", aug)):
        if t is None and name == "aug":
            continue
        if t.dtype != torch.int32 or t.dim() not in (1, 2) or t.stride(-1) != 1 or \
                t.shape[-1] != int(steps) * batch or (t.dim() == 2 and t.shape[0] != n_agents):
            raise ValueError(f"{name} must be int32 [{n_agents}, steps * batch] or "
                             "[steps * batch]")
    if targets is not None and (targets.dtype != torch.int32 or targets.dim() != 1 or
                                targets.shape[0] != n or not targets.is_contiguous()):
        raise ValueError("targets must be contiguous int32 [n]")
    if labels is not None and (labels.dtype != torch.int32 or labels.stride(1) != 1 or
                               tuple(labels.shape) != (n_agents, batch)):
        raise ValueError(f"labels must be int32 [{n_agents}, {batch}]")
    if cursor is not None and (cursor.dtype != torch.int32 or cursor.numel() != 1):
        raise ValueError("cursor must be one int32")
    for t in (index, aug, lut, targets, labels, cursor, data):
        if t is not None and t.device != samples.device:
            raise ValueError("every operand must live on the samples' device")

    def agent_stride(t):
        return t.stride(0) if t.dim() == 2 and n_agents > 1 else 0
    args = _lib.DlImageBatchArgs(
        _lib.ptr(samples), samples.stride(0) if n > 1 else dim, _lib.ptr(targets), n, C, H, W,
        _lib.ptr(lut), _lib.ptr(index), agent_stride(index), _lib.ptr(aug),
        agent_stride(aug) if aug is not None else 0, int(pad), int(fill), n_agents, batch,
        int(steps), _lib.ptr(cursor), int(step), int(bool(advance)), _lib.ptr(data),
        data.stride(0) if n_agents > 1 else batch * dim, _lib.ptr(labels),
        (labels.stride(0) if n_agents > 1 else batch) if labels is not None else 0)
    with torch.cuda.device(samples.device):
        _lib.check(_lib.load().dl_image_batch(ctypes.byref(args),
                                              _lib.stream_handle(samples.device)),
                   "dl_image_batch")
    return data


class BatchSampler:
    """Every agent's ``DataLoader`` over its ``random_split`` shard (Man_Colab.ipynb cell 16),
    with the dataset resident in HBM: ``next_into`` gathers all agents' next mini-batches in one
    ``dl_batch_gather`` launch and steps a cursor on the device, so a captured training step
    walks the epoch with no host work.

    samples: [n, ...] (flattened to fp32 [n, dim], dim % 4 == 0); targets: [n] class ids or
    None.  shards: one id list per agent; by default the reference's split, ``n // N`` ids each
    and the remainder to the last agent, cut from a permutation seeded by ``seed``.
    ``steps = min_a(len(shard_a)) // batch`` batches make an epoch: only full batches are used
    (the fused gradient kernel needs batch == 64), whereas the reference's ``epoch_len =
    min(len(loader))`` counts a short last batch too -- an epoch here is one step shorter
    whenever the smallest shard is no multiple of the batch.
    ``new_epoch()`` draws a fresh permutation of every shard on the device (``shuffle=True``) and
    keeps its first steps * batch ids; it rewrites the [N, steps * batch] int32 table in place and
    zeroes the cursor, so captured graphs stay valid.  ``batch_ids(step)`` are the ids a step
    uses, in agent order."""

    def __init__(self, samples, targets, n_agents, batch, shards=None, seed=0, device=None):
        import torch
        dev = self._resolve_device(samples, device)
        n = int(samples.shape[0])
        self._check_sizes(n_agents, batch)
        self.samples = samples.reshape(n, -1).to(dev, torch.float32).contiguous()
        self.dim = int(self.samples.shape[1])
        if self.dim % 4:
            raise ValueError("the sample length must be a multiple of 4")
        self._init_tables(n, targets, shards, seed)
        self.new_epoch()

    def _resolve_device(self, samples, device):
        import torch
        self._torch = torch
        dev = torch.device(device) if device is not None else (
            samples.device if samples.is_cuda else torch.device("cuda"))
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        return dev

    def _check_sizes(self, n_agents, batch):
        self.n_agents, self.batch = int(n_agents), int(batch)
        if self.n_agents < 1 or self.batch < 1:
            raise ValueError("n_agents and batch must be >= 1")

    def _init_tables(self, n, targets, shards, seed):
        """Targets, shards, the epoch table and the cursor (everything but the samples)."""
        torch, dev = self._torch, self.device
        self.targets = None
        if targets is not None:
            if targets.shape != (n,):
                raise ValueError("targets must be [n]")
            self.targets = targets.to(dev, torch.int32).contiguous()
        if shards is None:
            shards = self.default_shards(n, self.n_agents, seed)
        shards = [torch.as_tensor(s, dtype=torch.int64).reshape(-1) for s in shards]
        if len(shards) != self.n_agents:
            raise ValueError("one shard per agent")
        for s in shards:
            if s.numel() and (int(s.min()) < 0 or int(s.max()) >= n):
                raise ValueError("shard ids must lie in [0, n)")
        self.shards = shards
        lens = [int(s.numel()) for s in shards]
        self.steps = min(lens) // self.batch
        if self.steps < 1:
            raise ValueError(f"the smallest shard ({min(lens)} samples) holds no full batch of "
                             f"{self.batch}")
        # agent-order shards padded to one length; a padding slot's sort key is +inf, so a
        # permutation's first len(shard) entries are the shard's own
        pad = torch.zeros(self.n_agents, max(lens), dtype=torch.int32)
        for a, s in enumerate(shards):
            pad[a, :lens[a]] = s.to(torch.int32)
        self._ids = pad.to(dev)
        self._is_pad = (torch.arange(max(lens))[None, :] >=
                        torch.tensor(lens)[:, None]).to(dev)
        self._gen = torch.Generator(device=dev).manual_seed(int(seed))
        self.row_agent = None     # table row s holds agent row_agent[s]'s ids (None: agent s's)
        self.table = torch.zeros(self.n_agents, self.steps * self.batch, dtype=torch.int32,
                                 device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self.epochs = 0

    @staticmethod
    def default_shards(n, n_agents, seed=0):
        """The reference's split (cell 16): ``n // n_agents`` ids each, the remainder to the
        last agent, consecutive runs of a permutation seeded by ``seed``."""
        import torch
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))
        sizes = [n // n_agents] * n_agents
        sizes[-1] += n % n_agents
        return list(torch.split(perm, sizes))

    def attach_order(self, order):
        """Store agent order[s]'s ids in table row s from now on (an engine row order); the
        permutations drawn per agent do not change."""
        torch = self._torch
        if self.row_agent is not None:
            raise RuntimeError("the sampler already follows a row order")
        order = torch.as_tensor(order, dtype=torch.int64, device=self.device)
        self.table.copy_(self.table.index_select(0, order))
        self.row_agent = order

    def new_epoch(self):
        torch = self._torch
        keys = torch.rand(self._ids.shape, generator=self._gen, device=self.device,
                          dtype=torch.float64)
        keys.masked_fill_(self._is_pad, float("inf"))
        perm = torch.argsort(keys, dim=1)[:, :self.steps * self.batch]
        ids = torch.gather(self._ids, 1, perm)
        self.table.copy_(ids if self.row_agent is None else ids.index_select(0, self.row_agent))
        self.cursor.zero_()
        self.epochs += 1

    def batch_ids(self, step):
        """int64 [N, batch]: the sample ids of step ``step`` (mod steps) of the current epoch,
        row a agent a's."""
        s = int(step) % self.steps
        rows = self.table[:, s * self.batch:(s + 1) * self.batch].long()
        if self.row_agent is None:
            return rows
        out = self._torch.empty_like(rows)
        out[self.row_agent] = rows
        return out

    def next_into(self, data, labels=None):
        """Gather the batch the cursor points at into data [N, batch, dim] (and labels
        [N, batch] int32), rows in table order, then step the cursor."""
        return batch_gather(self.samples, self.table, data, targets=self.targets, labels=labels,
                            steps=self.steps, cursor=self.cursor, advance=True)


class ImageBatchSampler(BatchSampler):
    """``BatchSampler`` for a ``uint8`` image dataset under the reference's transforms
    (Man_Colab.ipynb cell 16): ``RandomCrop(H, padding=pad)``, ``RandomHorizontalFlip()`` (with
    ``flip``), ``ToTensor()`` and ``Normalize(mean, std)`` -- with pad = 0 and no flip, the test
    transform.  The dataset stays ``uint8`` in HBM (a quarter of the fp32 copy) and ``next_into``
    is one ``dl_image_batch`` launch that gathers, crops, flips and converts every agent's next
    mini-batch to fp32 [N, batch, C, H, W] (or [N, batch, C*H*W]: ``dim`` = C*H*W, so
    ``MLPConsensusSGD(sampler=...)`` takes it as it takes a ``BatchSampler``).

    Normalisation is the table ``lut[c][v] = (v / 255 - mean[c]) / std[c]`` computed in fp32 as
    torchvision computes a pixel, so the result equals ``ToTensor`` + ``Normalize`` bit for bit.
    The random draws are data: ``aug`` is an int32 table shaped like ``table`` (top in bits 0-7,
    left in bits 8-15, flip in bit 16), and ``new_epoch()`` -- which draws ``table`` exactly as
    ``BatchSampler`` does for the same seed and shards -- rewrites it in place from a second
    device generator derived from the seed: top, left ~ U{0..2 * pad}, flip ~ Bernoulli(1/2).
    ``aug_draws(step)`` are a step's draws in agent order, the twin of ``batch_ids``."""

    _AUG_SEED = 0x5DEECE66D

    def __init__(self, images_u8, targets, n_agents, batch, mean, std, pad=0, flip=False,
                 shards=None, seed=0, device=None):
        import torch
        dev = self._resolve_device(images_u8, device)
        if images_u8.dim() != 4 or images_u8.dtype != torch.uint8:
            raise ValueError("images must be uint8 [n, C, H, W]")
        n, C, H, W = (int(v) for v in images_u8.shape)
        self._check_sizes(n_agents, batch)
        if W % 4:
            raise ValueError("the image width must be a multiple of 4")
        if not 0 <= int(pad) <= 127:
            raise ValueError("pad must lie in [0, 127]")
        self.samples = images_u8.to(dev).contiguous()
        self.shape, self.dim = (C, H, W), C * H * W
        self.pad, self.flip, self.fill = int(pad), bool(flip), 0
        m = torch.as_tensor(mean, dtype=torch.float32).reshape(-1)
        sd = torch.as_tensor(std, dtype=torch.float32).reshape(-1)
        if m.numel() != C or sd.numel() != C:
            raise ValueError("one mean and one std per channel")
        # ToTensor: byte -> float32 / 255; Normalize: sub_(mean).div_(std), all in fp32
        self.lut = ((torch.arange(256, dtype=torch.float32).div(255)[None, :] - m[:, None]) /
                    sd[:, None]).contiguous().to(dev)
        self._init_tables(n, targets, shards, seed)
        self._aug_gen = torch.Generator(device=dev).manual_seed(int(seed) ^ self._AUG_SEED)
        self.aug = torch.zeros_like(self.table)
        self.new_epoch()

    def attach_order(self, order):
        """Store agent order[s]'s ids and draws in row s of both tables from now on."""
        super().attach_order(order)
        self.aug.copy_(self.aug.index_select(0, self.row_agent))

    def new_epoch(self):
        torch = self._torch
        super().new_epoch()
        shape, kw = tuple(self.table.shape), dict(generator=self._aug_gen, device=self.device,
                                                  dtype=torch.int32)
        top = torch.randint(0, 2 * self.pad + 1, shape, **kw)
        left = torch.randint(0, 2 * self.pad + 1, shape, **kw)
        words = top | (left << 8)
        if self.flip:
            words |= torch.randint(0, 2, shape, **kw) << 16
        self.aug.copy_(words if self.row_agent is None else
                       words.index_select(0, self.row_agent))

    def aug_draws(self, step):
        """(top, left, flip), each int64 [N, batch]: the draws of step ``step`` (mod steps) of
        the current epoch, row a agent a's."""
        s = int(step) % self.steps
        rows = self.aug[:, s * self.batch:(s + 1) * self.batch].long()
        if self.row_agent is not None:
            out = self._torch.empty_like(rows)
            out[self.row_agent] = rows
            rows = out
        return rows & 255, (rows >> 8) & 255, (rows >> 16) & 1

    def eval_transform(self, images_u8):
        """The test transform (``ToTensor`` + ``Normalize``) of uint8 [..., C, H, W] images
        through the same table: fp32 of the same shape, on the sampler's device."""
        torch = self._torch
        C = self.shape[0]
        x = images_u8.to(self.device)
        if x.dtype != torch.uint8 or x.dim() < 3 or x.shape[-3] != C:
            raise ValueError(f"images must be uint8 [..., {C}, H, W]")
        ch = torch.arange(C, device=self.device).view(C, 1, 1)
        return self.lut[ch, x.long()]

    def next_into(self, data, labels=None):
        """Transform the batch the cursor points at into data [N, batch, C, H, W] or
        [N, batch, C*H*W] (and labels [N, batch] int32), rows in table order, then step the
        cursor."""
        return image_batch(self.samples, self.table, data, self.lut, aug=self.aug, pad=self.pad,
                           fill=self.fill, targets=self.targets, labels=labels,
                           steps=self.steps, cursor=self.cursor, advance=True)


class MLPConsensusSGD:
    """Config c3 (BASELINE.json): every agent trains its own ``ANNModel`` (networks/ann_model.py)
    on its own batch and the agents mix after every local step -- the training loop of the
    reference's consensus notebooks (Man_Colab.ipynb cells 12-23: local SGD step, then
    ``Mixer.mix``), with all agents resident in HBM.

    One ``step()`` = batched per-agent gradients followed by the round X <- W (X - lr G) and the
    disagreement (``GossipEngine.round``).  emit="grad" (default): the kernel writes G and the
    fused round forms X - lr G on the fly (reads X and G).  emit="step" (fused kernel only): the
    gradient kernel writes the local step T = X - lr G itself and the round mixes T -- one matrix
    read instead of two, bit-identical X' -- but the kernel must then read every parameter again
    where its gradient is stored, and fc1.weight (72 % of them) is long out of the caches by
    then: at c3 the round saves 22 us and the gradient kernel loses 58 (3159 vs 3503 steps/s,
    PMC bytes per step 975 vs 985 MB; profiles/r10/c3_step).  ``G`` holds whichever was
    written.  Every call
    is stream-ordered with no host synchronisation, so ``capture()`` can record a step as a
    hipGraph (two graphs: the engine ping-pongs X/Y) and ``replay()`` then runs steps with one
    graph launch each instead of ~15 kernel launches from Python.

    sampler (a ``BatchSampler``, or an ``ImageBatchSampler`` over ``uint8`` images of din bytes;
    data and labels are then None): every step trains on the next
    mini-batch of each agent's shard instead of one fixed batch -- ``step()`` starts with
    ``sampler.next_into`` (one ``dl_batch_gather`` launch into buffers this object owns, the
    cursor on the device, so captured graphs walk the epoch by themselves) and ``fit`` runs
    whole epochs: the reference's ``MasterNode`` loop over every node's ``train_loader``.
    momentum / weight_decay / dampening / nesterov: the optimizer of Man_Colab.ipynb cell 19
    (``optim.SGD(momentum=0.9, weight_decay=5e-4)``) through ``GossipEngine.round_sgd`` with
    momentum buffers ``M``; needs emit="grad", and ``capture()`` then needs one eager step first
    (the buffers hold the first gradient).  All zero (the default): the plain step x - lr g.
    tracking=True: gradient tracking instead of the plain step (``GossipEngine.round_track``:
    D <- W (D + G - G_old), X <- W (X - lr D)), which with a constant lr reaches the optimum of
    the summed loss where the plain round stalls at a bias set by how much the agents' shards
    differ.  ``G`` and ``G_alt`` then alternate: ``gradients()`` writes the buffer of the current
    parity and ``round()`` passes the other one as last step's gradient; the parity flips with the
    engine's X / Y, so ``capture()`` records one graph per parity as before.  Needs emit="grad"
    and no momentum / weight_decay.
    optimizer="adam": torch.optim.Adam as the agents' optimizer (``GossipEngine.round_adam`` with
    ``betas``, ``eps`` and ``weight_decay`` as Adam's L2 term; the engine owns the moments and the
    step count).  The step count lives on the device and every step ticks it, inside a captured
    graph too, so ``capture()`` needs no eager step first.  Needs emit="grad"; exclusive with
    ``tracking`` and with momentum / dampening / nesterov.  The default "sgd" is everything
    above."""

    def __init__(self, ann, eng, data, labels, lr, deviation=True, emit="auto", sampler=None,
                 momentum=0.0, weight_decay=0.0, dampening=0.0, nesterov=False, tracking=False,
                 optimizer="sgd", betas=(0.9, 0.999), eps=1e-8):
        if eng.layout == "tiled" and ann.path != "fused":
            raise ValueError("the layered gradients read X row-major: use GossipEngine("
                             "layout='rows') or the fused kernel")
        if eng.n != ann.N or eng.P < ann.P:
            raise ValueError("engine and model disagree on agents/params")
        import torch
        self.ann, self.eng = ann, eng
        self.sampler = sampler
        if sampler is not None:
            if data is not None or labels is not None:
                raise ValueError("a sampler provides data and labels: pass None for both")
            if (sampler.n_agents, sampler.batch, sampler.dim) != (ann.N, ann.B, ann.din) or \
                    sampler.targets is None or sampler.device != eng.device:
                raise ValueError("the sampler must hold labelled samples of the model's input "
                                 "size for the engine's agents, batch and device")
            # rows of the batch buffers are engine rows: the table follows the row order once
            if eng.order is not None:
                sampler.attach_order(eng.order)
            data = torch.empty(ann.N, ann.B, ann.din, dtype=torch.float32, device=eng.device)
            labels = torch.empty(ann.N, ann.B, dtype=torch.int32, device=eng.device)
        # an engine row order (GossipEngine(order=...), "auto" on plan-path-5 graphs) stores
        # agent eng.order[s] in row s: every per-agent input follows it, so each row still
        # trains on its own agent's batch (results per agent are those of agent order)
        elif eng.order is not None:
            data = data.index_select(0, eng.order.to(data.device))
            labels = labels.index_select(0, eng.order.to(labels.device))
        self.data, self.labels = data, labels
        self.lr, self.deviation = float(lr), bool(deviation)
        if emit == "auto":
            emit = "grad"
        if emit not in ("step", "grad") or (emit == "step" and ann.path != "fused"):
            raise ValueError("emit must be 'grad', or 'step' with the fused gradient kernel")
        self.emit = emit
        if optimizer not in ("sgd", "adam"):
            raise ValueError(f"optimizer must be 'sgd' or 'adam' (got {optimizer!r})")
        self.adam = optimizer == "adam"
        if self.adam and tracking:
            raise ValueError("optimizer='adam' and tracking=True are exclusive: gradient tracking "
                             "steps along the tracker with the plain step")
        if self.adam and (momentum != 0.0 or dampening != 0.0 or nesterov or emit != "grad"):
            raise ValueError("optimizer='adam' needs emit='grad' and takes betas / eps / "
                             "weight_decay, not momentum / dampening / nesterov")
        self.tracking = bool(tracking)
        if self.tracking and (momentum != 0.0 or weight_decay != 0.0 or emit != "grad"):
            raise ValueError("tracking needs emit='grad' and no momentum / weight_decay")
        self.opt = dict(momentum=float(momentum), dampening=float(dampening),
                        weight_decay=float(weight_decay), nesterov=bool(nesterov))
        self.optimizer = not self.adam and (momentum != 0.0 or weight_decay != 0.0)
        self.adam_opt = dict(betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                             weight_decay=float(weight_decay))
        if self.optimizer and emit != "grad":
            raise ValueError("momentum / weight_decay need emit='grad'")
        self.M = torch.zeros_like(eng.X) if momentum != 0.0 else None
        self.steps_done = 0
        # Row-major engines may carry zero padding columns [ann.P, eng.P) (a whole number of mix
        # tiles: no ragged tail launch); the tiled layout zero-pads its last tile itself.  Padding
        # stays exactly zero -- G is zero there and W 0 = 0 -- and adds exact zeros to the
        # deviation, so results are those of the unpadded round.
        self.G = torch.zeros_like(eng.X)
        # tracking: the gradient buffer of the other parity (last step's gradient; zero at first)
        self.G_alt = torch.zeros_like(eng.X) if self.tracking else None
        self._gpar = 0
        if self.tracking:
            eng.reset_tracker()
        if self.adam:
            eng.reset_adam(self.lr, self.adam_opt["betas"])
        self.graphs = None
        self._torch = torch

    @property
    def loss(self):
        """Per-row mean cross-entropy of the last step (device tensor [N]; row s is agent
        ``eng.order[s]`` under an engine row order, see ``agent_loss``)."""
        return self.ann.loss

    def agent_loss(self):
        """Per-agent mean cross-entropy of the last step, in agent order."""
        if self.eng.order is None:
            return self.ann.loss
        out = self._torch.empty_like(self.ann.loss)
        out[self.eng.order] = self.ann.loss
        return out

    def evaluate(self, data, labels, logits=None, row_splits=0):
        """Every agent's current model on a test set (``BatchedANN.evaluate`` on ``eng.X`` in
        whichever layout it has): (loss[N], correct[N]) in agent order -- the reference's
        per-node test statistics (Man_Colab.ipynb cells 21-23).  data: [R, din] shared by all
        agents or [N, R, din] per agent; labels: int32 [R] or [N, R]; per-agent inputs and the
        optional logits [N, R, dout] are in agent order too.  Stream-ordered, no host
        synchronisation: capturable in a hipGraph."""
        order = self.eng.order
        if order is not None:      # row s holds agent order[s]
            if data.dim() == 3:
                data = data.index_select(0, order.to(data.device))
            if labels is not None and labels.dim() == 2:
                labels = labels.index_select(0, order.to(labels.device))
        rows_logits = logits if order is None or logits is None else \
            self._torch.empty_like(logits)
        X = self.eng.X if self.eng.layout == "tiled" else self.eng.X[:, :self.ann.P]
        loss, correct = self.ann.evaluate(X, data, labels, logits=rows_logits,
                                          row_splits=row_splits)
        if order is None:
            return loss, correct
        if logits is not None:
            logits[order] = rows_logits
        if loss is None:
            return None, None
        out = self._torch.empty_like(loss), self._torch.empty_like(correct)
        out[0][order] = loss
        out[1][order] = correct
        return out

    @staticmethod
    def padded_params(csr, n_params, device):
        """n_params rounded up to the row-major mix tile width for this graph."""
        from .engine import DeviceCsr, plan_shape
        T = plan_shape(DeviceCsr(csr, device), n_params, deviation=True)["tile_cols"]
        return -(-n_params // T) * T if T else n_params

    def gradients(self):
        """The gradient phase alone: G (emit="grad") or T = X - lr G (emit="step")."""
        P = self.ann.P
        lr = self.lr if self.emit == "step" else None
        G = self._g_now()
        if self.eng.layout == "tiled":     # the fused kernel addresses the tiles directly
            self.ann.gradients(self.eng.X, self.data, self.labels, G, lr=lr)
        else:
            self.ann.gradients(self.eng.X[:, :P], self.data, self.labels, G[:, :P], lr=lr)

    def _g_now(self):
        """The gradient buffer ``gradients()`` writes: ``G``, or with tracking the one of the
        current parity."""
        return self.G_alt if self._gpar else self.G

    def round(self):
        """The round phase alone (after ``gradients``)."""
        if self.tracking:
            g_old = self.G if self._gpar else self.G_alt
            self.eng.round_track(self._g_now(), g_old, self.lr, deviation=self.deviation)
            self._gpar ^= 1
        elif self.adam:
            self.eng.round_adam(self.G, self.lr, deviation=self.deviation, **self.adam_opt)
        elif self.optimizer:
            self.eng.round_sgd(self.G, self.M, self.lr, first=self.steps_done == 0,
                               deviation=self.deviation, **self.opt)
        elif self.emit == "step":
            self.eng.round(src=self.G, deviation=self.deviation)
        else:
            self.eng.round(G=self.G, lr=self.lr, deviation=self.deviation)

    def step(self):
        if self.sampler is not None:
            self.sampler.next_into(self.data, self.labels)
        self.gradients()
        self.round()
        self.steps_done += 1

    def capture(self):
        """Record one step per ping-pong parity.  Runs nothing: the engine state afterwards is
        what it was before (and so are the sampler's cursor and the step count)."""
        torch = self._torch
        if self.optimizer and self.steps_done == 0:
            raise RuntimeError("run one eager step before capture(): the first step of "
                               "momentum SGD differs from the ones a graph replays")
        self.eng.reserve_workspace(self.deviation)
        done = self.steps_done
        # (recording a step advances the host mirror of Adam's step count, not the device's)
        adam_host = (self.eng.adam.t, self.eng.adam.b1t, self.eng.adam.b2t) if self.adam else None
        graphs = []
        for _ in range(2):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.step()               # records; swaps eng.X / eng.Y on the host
            graphs.append(g)
        self.graphs = graphs              # two swaps: eng.X is the original buffer again
        self._parity = 0
        self.steps_done = done
        if self.adam:
            self.eng.adam.t, self.eng.adam.b1t, self.eng.adam.b2t = adam_host

    def replay(self, steps=1):
        for _ in range(int(steps)):
            self.graphs[self._parity].replay()
            self._parity ^= 1
            self.eng.X, self.eng.Y = self.eng.Y, self.eng.X
            if self.tracking:
                self._gpar ^= 1
            if self.adam:
                self.eng.adam.advance_host()
            self.steps_done += 1

    def fit(self, epochs, stat_step=None, test=None):
        """``epochs`` epochs over the sampler's shards: per epoch ``sampler.new_epoch()`` and
        then ``sampler.steps`` steps (graph replays after ``capture()``, else eager steps).
        Every ``stat_step`` steps, counted from this call's start, ``evaluate(*test)`` -- the
        reference's per-node statistics every ``stat_step`` -- is appended to the returned
        history as (step, loss[N], correct[N])."""
        if self.sampler is None:
            raise ValueError("fit needs a sampler")
        if stat_step is not None and (int(stat_step) < 1 or test is None):
            raise ValueError("stat_step must be >= 1 and needs a test set")
        history, step = [], 0
        for _ in range(int(epochs)):
            self.sampler.new_epoch()
            for _ in range(self.sampler.steps):
                if self.graphs is not None:
                    self.replay()
                else:
                    self.step()
                step += 1
                if stat_step is not None and step % int(stat_step) == 0:
                    loss, correct = self.evaluate(*test)
                    history.append((step, loss.clone(), correct.clone()))
        return history


def _sgd_args(X, G, M, out, lr, momentum, dampening, weight_decay, nesterov, first):
    from . import _lib
    return _lib.DlSgdArgs(_lib.ptr(X), X.stride(0), _lib.ptr(G), G.stride(0), _lib.ptr(M),
                          M.stride(0) if M is not None else 0, _lib.ptr(out), out.stride(0),
                          X.shape[0], X.shape[1], float(lr), float(momentum), float(dampening),
                          float(weight_decay), int(bool(nesterov)), int(bool(first)))


def sgd_step(X, G, M=None, out=None, lr=0.1, momentum=0.0, dampening=0.0, weight_decay=0.0,
             nesterov=False, first=False):
    """``dl_sgd_step``: torch.optim.SGD.step over agent rows (X, G, M, out: [N, P] row-major
    device tensors; out defaults to X, i.e. in place).  Stream-ordered, no host sync."""
    import ctypes

    from . import _lib
    out = X if out is None else out
    for name, t in (("X", X), ("G", G), ("M", M), ("out", out)):
        if t is None:
            continue
        if t.dtype.itemsize != 4 or not t.is_floating_point() or t.dim() != 2 or \
                t.stride(1) != 1 or tuple(t.shape) != tuple(X.shape) or t.device != X.device:
            raise ValueError(f"{name} must be a row-major float32 [N, P] tensor like X")
    if momentum != 0.0 and M is None:
        raise ValueError("momentum needs a buffer M")
    args = _sgd_args(X, G, M, out, lr, momentum, dampening, weight_decay, nesterov, first)
    _lib.check(_lib.load().dl_sgd_step(ctypes.byref(args), _lib.stream_handle(X.device)),
               "dl_sgd_step")
    return out


def wrn_flops_per_image(depth=16, widen=4, num_classes=10, hw=32):
    """Forward FLOPs of one image through Wide_ResNet (convs + linear, 2 per MAC), and the FLOPs of
    forward + backward (input and weight gradients; the first conv needs no input gradient)."""
    n = (depth - 4) // 6
    st = [16, 16 * widen, 32 * widen, 64 * widen]
    convs = [(3, st[0], 3, hw)]               # (cin, cout, k, output hw)
    cin, h = st[0], hw
    for i, s in enumerate([1, 2, 2]):
        for j in range(n):
            stride = s if j == 0 else 1
            cout = st[i + 1]
            ho = h // stride
            convs.append((cin, cout, 3, h))           # conv1 (stride 1)
            convs.append((cout, cout, 3, ho))         # conv2 (strided)
            if stride != 1 or cin != cout:
                convs.append((cin, cout, 1, ho))      # 1x1 shortcut
            cin, h = cout, ho
    fwd = [2 * ci * co * k * k * o * o for ci, co, k, o in convs] + [2 * st[3] * num_classes]
    total = sum(fwd)
    return total, total + 2 * total - fwd[0]


class WRNConsensusSGD:
    """Config c5 (BASELINE.json): every agent trains its own Wide-ResNet (WRN-16-4,
    networks/wide_resnet.py) with the optimizer of Man_Colab.ipynb cell 19 (SGD, momentum 0.9,
    weight decay 5e-4, lr 0.02) on its own CIFAR-shaped batch, and the agents mix after every
    local step (the ``MasterNode`` loop the notebook drives, cells 21-23: local step, then
    ``Mixer.mix``, mixer.py:18-49).

    Layout: all agents' parameters are the rows of one row-major X[N, P] in HBM -- the Mixer's
    flatten order (mixer.py:68-69) -- and every agent's ``nn.Module`` parameters are views of its
    row; their ``.grad`` are views of G's rows, so backward accumulates straight into G.  One
    ``step()``:
      1. G = 0; per agent: forward, cross-entropy, backward (PyTorch-ROCm convs, MIOpen), agents
         spread round-robin over ``streams`` HIP streams;
      2. ``dl_sgd_step``: torch.optim.SGD's update (momentum buffers M), written to the scratch
         S instead of in place;
      3. ``dl_mix_round``: X <- W S with the fused disagreement -- the parameters land back in
         X, so the module views never move and no copy or re-binding is needed.
    ``fused_round=True`` runs 2 and 3 as one ``dl_sgd_round`` on X in place (the same bits, 20
    instead of 28 B per element across HBM) and allocates no S.
    Every call is stream-ordered: ``capture()`` records a step as one hipGraph.

    sampler (an ``ImageBatchSampler``; data and labels are then None): every step trains on the
    next augmented mini-batch of each agent's shard instead of one fixed batch -- the reference's
    ``train_loader`` under ``transform_train`` (Man_Colab.ipynb cell 16).  ``step()`` then starts
    with ``sampler.next_into`` (one ``dl_image_batch`` launch into fp32 [N, B, C, H, W] data and
    int32 labels this object owns, the cursor on the device) and one copy of the labels into the
    int64 tensor ``F.cross_entropy`` needs, both inside the captured graph, and ``fit`` runs whole
    epochs."""

    def __init__(self, csr, batch, depth=16, widen=4, dropout=0.0, num_classes=10, lr=0.02,
                 momentum=0.9, weight_decay=5e-4, device="cuda", X0=None, seed=0, streams=1,
                 deviation=True, data=None, labels=None, fused_round=False, sampler=None):
        import torch

        from .engine import DeviceCsr, Workspace, plan_shape, sgd_round_plan
        from .networks.wide_resnet import Wide_ResNet
        self._torch = torch
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.N, self.B = csr.n_rows, int(batch)
        self.lr, self.momentum, self.wd = float(lr), float(momentum), float(weight_decay)
        self.deviation = bool(deviation)
        self.arch = (int(depth), int(widen), float(dropout), int(num_classes))
        self.models = []
        with torch.random.fork_rng(devices=[]):     # default torch init, agent a seeded seed + a
            for a in range(self.N):
                torch.manual_seed(seed + a)
                self.models.append(Wide_ResNet(*self.arch).to(self.device))
        shapes = [p.shape for p in self.models[0].parameters()]
        self.P = sum(int(np.prod(s)) for s in shapes)
        self.W = DeviceCsr(csr, self.device)
        T = plan_shape(self.W, self.P, deviation=True)["tile_cols"] or 1
        self.ld = -(-self.P // max(T, 16)) * max(T, 16)   # zero padding: no ragged tail launch
        f = lambda: torch.zeros(self.N, self.ld, dtype=torch.float32, device=self.device)  # noqa
        self.X, self.G = f(), f()
        self.M = f() if self.momentum != 0.0 else None
        # fused_round: steps 2 and 3 as one in-place dl_sgd_round on X, no scratch S -- where the
        # fused kernel takes this graph and shape; else the two launches
        self.fused_round = bool(fused_round) and sgd_round_plan(
            self.W, self.X, self.X, self.G, self.M, momentum=self.momentum,
            weight_decay=self.wd, deviation=self.deviation) is not None
        self.S = None if self.fused_round else f()
        with torch.no_grad():
            for a, m in enumerate(self.models):
                if X0 is None:
                    self.X[a, :self.P] = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
                else:
                    self.X[a, :self.P] = torch.as_tensor(X0[a], dtype=torch.float32)
                off = 0
                for p in m.parameters():
                    n = p.numel()
                    p.set_(self.X[a, off:off + n].view_as(p))
                    p.grad = self.G[a, off:off + n].view_as(p)
                    off += n
        self.dev_sq = torch.zeros(self.N, dtype=torch.float32, device=self.device)
        self.dev_max = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.loss = torch.zeros(self.N, dtype=torch.float32, device=self.device)
        self.ws = Workspace(self.device)
        self.sampler, self.labels32 = sampler, None
        if sampler is not None:
            if data is not None or labels is not None:
                raise ValueError("a sampler provides data and labels: pass None for both")
            if (sampler.n_agents, sampler.batch) != (self.N, self.B) or \
                    sampler.targets is None or sampler.device != self.device or \
                    len(getattr(sampler, "shape", ())) != 3:
                raise ValueError("the sampler must hold labelled images for this graph's "
                                 "agents, batch and device")
            data = torch.empty(self.N, self.B, *sampler.shape, dtype=torch.float32,
                               device=self.device)
            self.labels32 = torch.empty(self.N, self.B, dtype=torch.int32, device=self.device)
            labels = torch.empty(self.N, self.B, dtype=torch.int64, device=self.device)
        elif data is None:
            g = torch.Generator(device=self.device).manual_seed(seed)
            data = torch.randn(self.N, self.B, 3, 32, 32, device=self.device, generator=g)
            labels = torch.randint(0, num_classes, (self.N, self.B), device=self.device,
                                   generator=g)
        self.data, self.labels = data, labels
        self.n_streams = max(1, int(streams))
        self.streams = [torch.cuda.Stream(self.device) for _ in range(self.n_streams)] \
            if self.n_streams > 1 else []
        self.steps_done = 0
        self.graph = None

    def params(self):
        """Row-major [N, P] view of every agent's flattened parameters (Mixer order)."""
        return self.X[:, :self.P]

    def flops_per_step(self):
        return wrn_flops_per_image(self.arch[0], self.arch[1], self.arch[3])[1] * self.N * self.B

    def _local_grads(self):
        torch = self._torch
        F = torch.nn.functional
        self.G.zero_()
        main = torch.cuda.current_stream(self.device)
        for s in self.streams:
            s.wait_stream(main)
        for a, m in enumerate(self.models):
            ctx = torch.cuda.stream(self.streams[a % self.n_streams]) if self.streams else \
                _nullctx()
            with ctx:
                loss = F.cross_entropy(m(self.data[a]), self.labels[a])
                loss.backward()
                self.loss[a:a + 1].copy_(loss.detach().reshape(1))
        for s in self.streams:
            main.wait_stream(s)

    def _round(self, first):
        from .engine import mix_round, sgd_round
        dev = dict(dev_sq=self.dev_sq if self.deviation else None,
                   dev_max=self.dev_max if self.deviation else None, workspace=self.ws)
        if self.fused_round and sgd_round(self.W, self.X, self.X, self.G, self.M, self.lr,
                                          momentum=self.momentum, weight_decay=self.wd,
                                          first=first, **dev):
            return
        if self.S is None:   # (the plan at construction took the round: not reached)
            self.S = self._torch.zeros_like(self.X)
        sgd_step(self.X, self.G, self.M, out=self.S, lr=self.lr, momentum=self.momentum,
                 weight_decay=self.wd, first=first)
        mix_round(self.W, self.S, self.X, **dev)

    def _next_batch(self):
        """With a sampler: every agent's next augmented mini-batch and its int64 labels."""
        if self.sampler is not None:
            self.sampler.next_into(self.data, self.labels32)
            self.labels.copy_(self.labels32)

    def step(self):
        self._next_batch()
        self._local_grads()
        self._round(first=self.steps_done == 0)
        self.steps_done += 1

    def fit(self, epochs):
        """``epochs`` epochs over the sampler's shards: per epoch ``sampler.new_epoch()`` and
        then ``sampler.steps`` steps (graph replays after ``capture()``, else eager steps)."""
        if self.sampler is None:
            raise ValueError("fit needs a sampler")
        for _ in range(int(epochs)):
            self.sampler.new_epoch()
            for _ in range(self.sampler.steps):
                if self.graph is not None:
                    self.replay()
                else:
                    self.step()

    def capture(self):
        """Record one step (after at least one eager step: the momentum buffers exist and every
        MIOpen solution is found) as a hipGraph.  Runs nothing (the sampler's cursor stays where
        it is)."""
        torch = self._torch
        if self.steps_done == 0:
            raise RuntimeError("run one eager step before capture()")
        from . import _lib
        self.ws.get(_lib.load().dl_mix_workspace_bytes(self.N, 0, self.ld))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._next_batch()
            self._local_grads()
            self._round(first=False)
        self.graph = g

    def replay(self, steps=1):
        for _ in range(int(steps)):
            self.graph.replay()
            self.steps_done += 1


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
