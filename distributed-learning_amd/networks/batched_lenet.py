"""Batched per-agent LeNet gradients on the GPU: the model of the reference's CIFAR run
(Man_Colab.ipynb cell 19, ``model_name = 'lenet'``) with ``BatchedANN``'s interface.

All agents' parameters are rows of one matrix X[N, P] in the Mixer flatten order (conv1.w,
conv1.b, conv2.w, conv2.b, fc1.w, ..., fc3.b; mixer.py:69).  One ``gradients`` call is one
``dl_lenet_grad``: a fixed sequence of launches over every agent at once -- the convolution
stages as hand-written fp32 kernels (csrc/lenet.hip), the Linear layers and the cross-entropy
head as ``dl_bgemm``'s GEMMs -- with no per-agent Python loop and no autograd graph.  X and G are
row-major (``GossipEngine(layout="rows")``)."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .lenet import LeNet

IMAGE = 3 * 32 * 32


class BatchedLeNet:
    path = "layers"   # what MLPConsensusSGD asks of a model that reads X row-major

    def __init__(self, n_agents, batch, num_classes=10, device="cuda", fused_eval=False):
        self.N, self.B = int(n_agents), int(batch)
        self.fused_eval = bool(fused_eval)   # evaluate's default path: one dl_lenet_eval call
        self.din, self.dout = IMAGE, int(num_classes)
        if not 1 <= self.dout <= 64:
            raise ValueError("the cross-entropy head supports 1 to 64 classes")
        self.device = torch.device(device)
        self.offsets = {}
        off = 0
        for name, shape in LeNet.param_shapes(self.dout):
            self.offsets[name] = off
            off += int(np.prod(shape))
        self.P = off
        self.loss = torch.empty(self.N, dtype=torch.float32, device=self.device)
        # gradients' workspace, allocated on first use and never replaced: a captured step
        # holds its address.  evaluate has its own (it grows with the chunk), as BatchedANN's.
        self.ws = None
        self.eval_ws = self.eval_out = self.eval_logits = self.eval_acc = None
        self.fused_ws = self.fused_out = None   # dl_lenet_eval's workspace and (loss, correct)

    def _workspace(self, rows, evaluate=False):
        need = _lib.load().dl_lenet_workspace_bytes(self.N, int(rows), self.dout)
        ws = self.eval_ws if evaluate else self.ws
        if ws is None or ws.numel() * 4 < need:
            ws = torch.empty(-(-need // 4), dtype=torch.float32, device=self.device)
            if evaluate:
                self.eval_ws = ws
            else:
                self.ws = ws
        return _lib.ptr(ws), ws.numel() * 4

    def _check_rows(self, X, name="X"):
        if tuple(X.shape) != (self.N, self.P) or X.stride(1) != 1 or X.dtype != torch.float32:
            raise ValueError(f"{name}: expected a row-major fp32 [{self.N}, {self.P}] tensor")

    def gradients(self, X, data, labels, G, lr=None):
        """G[a] = d loss_a / d params_a for every agent.  X, G: [N, P] row-major fp32 (row stride
        a multiple of 4 that may exceed P, 16-byte aligned); data: contiguous fp32 [N, B, 3072] or
        [N, B, 3, 32, 32]; labels: int32 [N, B].  Returns the per-agent mean cross-entropy
        (device tensor [N], this object's ``loss``)."""
        if lr is not None:
            raise ValueError("the local-step output (lr=...) needs BatchedANN's fused kernel")
        N, B = self.N, self.B
        if tuple(data.shape) not in ((N, B, IMAGE), (N, B, 3, 32, 32)) or \
                not data.is_contiguous() or data.dtype != torch.float32:
            raise ValueError(f"data must be contiguous fp32 [{N}, {B}, {IMAGE}] or "
                             f"[{N}, {B}, 3, 32, 32]")
        if tuple(labels.shape) != (N, B) or labels.dtype != torch.int32 or labels.stride(1) != 1:
            raise ValueError(f"labels must be int32 [{N}, {B}]")
        self._check_rows(X)
        self._check_rows(G, "G")
        ws, ws_bytes = self._workspace(B)
        args = _lib.DlLenetArgs(N, B, self.dout, _lib.ptr(X), X.stride(0), _lib.ptr(data),
                                B * IMAGE, _lib.ptr(labels), labels.stride(0), _lib.ptr(G),
                                G.stride(0), _lib.ptr(self.loss), None, 0, 0)
        _lib.check(_lib.load().dl_lenet_grad(ctypes.byref(args), ws, ws_bytes,
                                             _lib.stream_handle(self.device)), "dl_lenet_grad")
        return self.loss

    def evaluate(self, X, data, labels, logits=None, row_splits=0, chunk=512, fused=None):
        """Every agent's model on a test set, forward only: returns (loss[N] fp32 mean
        cross-entropy, correct[N] int32 rows whose logit argmax is the label), the per-node
        statistics of the reference's MasterNode (Man_Colab.ipynb cells 21-23).

        data: contiguous fp32 [R, 3072] / [R, 3, 32, 32] (one test set shared by all agents) or
        with a leading [N]; labels: int32 [R] or [N, R] (None with ``logits`` alone); logits:
        optional fp32 [N, R, num_classes] output with a contiguous last dimension.  The rows go
        through the forward-only ``dl_lenet_grad`` in chunks of ``chunk``; the loss and the
        argmax come from each chunk's logits with torch ops, summed in fp64.  ``row_splits`` is
        accepted for ``BatchedANN``'s signature and ignored on this path.  The returned tensors
        are this object's, overwritten by the next call.

        Stream-ordered with no host synchronisation.  The workspace (separate from
        ``gradients``'), the logits chunk, the accumulators and the outputs are this object's and
        allocated on first use or when a larger chunk needs them; unlike ``BatchedANN.evaluate``
        the torch ops on each chunk's logits allocate their temporaries from torch's caching
        allocator on every call, which a ``torch.cuda.graph`` capture serves from the graph's
        pool.  A captured ``evaluate`` holds the addresses of its call: capture it after the
        largest chunk it will be asked for.

        fused (None: the constructor's ``fused_eval``) true: one ``dl_lenet_eval`` call for the
        whole test set instead -- the forward and the head in one kernel with the activations in
        LDS, then a block-order reduce (include/dlamd.h states the sum order).  ``row_splits`` is
        forwarded (0 = chosen; any value gives the same bits) and ``chunk`` ignored.  Once its
        buffers exist -- the outputs and a workspace of two numbers per 64 rows, allocated on
        first use and regrown only for more rows -- the call runs no torch op and allocates
        nothing: a capture is two kernels."""
        N, dout = self.N, self.dout
        per_agent = data.dim() in (3, 5)
        if data.dim() not in (2, 3, 4, 5) or data.dtype != torch.float32 or \
                not data.is_contiguous() or (per_agent and data.shape[0] != N) or \
                tuple(data.shape[1 + per_agent:]) not in ((IMAGE,), (3, 32, 32)):
            raise ValueError(f"data must be contiguous fp32 [R, {IMAGE}] or [R, 3, 32, 32], "
                             f"optionally with a leading [{N}]")
        R = int(data.shape[int(per_agent)])
        chunk = int(chunk)
        if R < 1 or chunk < 1:
            raise ValueError("data has no rows, or chunk < 1")
        s_data = R * IMAGE if per_agent else 0
        if labels is None:
            if logits is None:
                raise ValueError("nothing to compute: no labels and no logits buffer")
        elif labels.dtype != torch.int32 or tuple(labels.shape) not in ((R,), (N, R)):
            raise ValueError(f"labels must be int32 [{R}] or [{N}, {R}]")
        if logits is not None and (tuple(logits.shape) != (N, R, dout) or
                                   logits.dtype != torch.float32 or logits.stride(2) != 1 or
                                   logits.stride(1) < dout or
                                   (N > 1 and logits.stride(0) < R * logits.stride(1))):
            raise ValueError(f"logits must be fp32 [{N}, {R}, {dout}] with a contiguous last "
                             "dimension and non-overlapping rows")
        self._check_rows(X)
        if self.fused_eval if fused is None else fused:
            return self._evaluate_fused(X, data, s_data, R, labels, logits, row_splits)
        chunk = min(chunk, R)
        if logits is None:
            if self.eval_logits is None or self.eval_logits.shape[1] < chunk:
                self.eval_logits = torch.empty(N, chunk, dout, dtype=torch.float32,
                                               device=self.device)
            Z = self.eval_logits
        else:
            Z = logits
        lib = _lib.load()
        ws, ws_bytes = self._workspace(chunk, evaluate=True)
        if self.eval_acc is None:
            self.eval_acc = (torch.empty(N, dtype=torch.float64, device=self.device),
                             torch.empty(N, dtype=torch.int64, device=self.device))
        lsum, hits = self.eval_acc
        lsum.zero_()
        hits.zero_()
        for r0 in range(0, R, chunk):
            c = min(chunk, R - r0)
            z = Z[:, r0:r0 + c] if logits is not None else Z[:, :c]
            args = _lib.DlLenetArgs(N, c, dout, _lib.ptr(X), X.stride(0),
                                    ctypes.c_void_p(data.data_ptr() + 4 * r0 * IMAGE), s_data,
                                    None, 0, None, 0, None,
                                    ctypes.c_void_p(z.data_ptr()), z.stride(1), z.stride(0))
            _lib.check(lib.dl_lenet_grad(ctypes.byref(args), ws, ws_bytes,
                                         _lib.stream_handle(self.device)), "dl_lenet_grad")
            if labels is not None:
                lab = labels[..., r0:r0 + c].long().expand(N, c)
                zl = z.gather(2, lab.unsqueeze(2)).squeeze(2)
                lsum += (torch.logsumexp(z, 2) - zl).double().sum(1)
                hits += (z.argmax(2) == lab).sum(1)
        if labels is None:
            return None, None
        if self.eval_out is None:
            self.eval_out = (torch.empty(N, dtype=torch.float32, device=self.device),
                             torch.empty(N, dtype=torch.int32, device=self.device))
        loss, correct = self.eval_out
        loss.copy_(lsum / R)
        correct.copy_(hits)
        return loss, correct

    def _evaluate_fused(self, X, data, s_data, R, labels, logits, row_splits):
        lib = _lib.load()
        if labels is not None and labels.stride(-1) != 1:
            raise ValueError("labels must have a contiguous last dimension")
        if self.fused_ws is None or self.fused_ws[1] < R:
            need = lib.dl_lenet_eval_workspace_bytes(self.N, R)
            self.fused_ws = (torch.empty(need // 4, dtype=torch.float32, device=self.device), R)
        if self.fused_out is None:
            self.fused_out = (torch.empty(self.N, dtype=torch.float32, device=self.device),
                              torch.empty(self.N, dtype=torch.int32, device=self.device))
        loss, correct = self.fused_out if labels is not None else (None, None)
        ws = self.fused_ws[0]
        args = _lib.DlLenetEvalArgs(
            self.N, R, self.dout, _lib.ptr(X), X.stride(0), _lib.ptr(data), s_data,
            _lib.ptr(labels), labels.stride(0) if labels is not None and labels.dim() == 2 else 0,
            _lib.ptr(loss), _lib.ptr(correct), _lib.ptr(logits),
            logits.stride(1) if logits is not None else 0,
            logits.stride(0) if logits is not None else 0, int(row_splits))
        _lib.check(lib.dl_lenet_eval(ctypes.byref(args), _lib.ptr(ws), ws.numel() * 4,
                                     _lib.stream_handle(self.device)), "dl_lenet_eval")
        return loss, correct

    def flops_per_step(self):
        """Forward + backward FLOPs of one ``gradients`` call (conv1 has no input gradient)."""
        conv1, conv2 = 6 * 28 * 28 * 75, 16 * 10 * 10 * 150
        fc = 400 * 120 + 120 * 84 + 84 * self.dout
        return self.N * self.B * 2 * (2 * conv1 + 3 * conv2 + 3 * fc)
