"""BatchedANN.evaluate's host side, without a GPU: the shape gate of the one-launch evaluation
(the gradient kernel's without its batch clause) and the argument checks, which refuse bad
inputs before any device work."""
import pytest
import torch


def test_eval_gate_ignores_the_training_batch():
    from distributed_learning_amd.networks.batched_ann import (BatchedANN, eval_supported,
                                                                fused_supported)
    assert eval_supported(784, 150, 10) and eval_supported(16, 152, 16)
    assert not eval_supported(786, 150, 10)        # input_dim % 4
    assert not eval_supported(784, 151, 10)        # odd hidden
    assert not eval_supported(784, 154, 10)        # hidden > 152
    assert not eval_supported(784, 150, 17)        # classes > 16
    assert not eval_supported(50, 40, 7)
    # a model trained with batch 32 takes the layered gradients but the evaluation kernel
    assert not fused_supported(32, 784, 150, 10)
    b = BatchedANN(4, 32, device="cpu")
    assert b.path == "layers" and b.eval_ws is None and b.eval_out is None
    assert b.eval_flops(64) == 4 * 2 * 64 * (784 * 150 + 2 * 150 * 150 + 150 * 10)


def test_argument_checks():
    from distributed_learning_amd.networks.batched_ann import BatchedANN
    n, r, din, dout = 3, 10, 52, 7
    b = BatchedANN(n, 64, din, 40, dout, device="cpu")
    X = torch.zeros(n, b.P)
    data = torch.zeros(r, din)
    labels = torch.zeros(r, dtype=torch.int32)
    bad = [
        (X, data, labels.long()),                                   # label dtype
        (X, data, labels.float()),
        (X, torch.zeros(din), labels),                              # data rank
        (X, torch.zeros(1, n, r, din), labels),
        (X, torch.zeros(r, din + 4), labels),                       # data columns
        (X, torch.zeros(n + 1, r, din), labels),                    # agents
        (X, data.double(), labels),
        (X, torch.zeros(0, din), labels[:0]),                       # no rows
        (X, data, torch.zeros(r + 1, dtype=torch.int32)),           # label shape
        (X, data, torch.zeros(n + 1, r, dtype=torch.int32)),
        (X, data, None),                                            # nothing to compute
        (torch.zeros(n, b.P + 4), data, labels),                    # X shape
        (torch.zeros(5, n + 1, 64), data, labels),                  # tiled X: agents
        (torch.zeros(2, n, 64), data, labels),                      # tiled X: too few columns
    ]
    for args in bad:
        with pytest.raises(ValueError):
            b.evaluate(*args)
    for logits in (torch.zeros(n, r, dout + 1), torch.zeros(n, r, dout, dtype=torch.float64),
                   torch.zeros(n, r, 2 * dout)[:, :, ::2], torch.zeros(r, dout)):
        with pytest.raises(ValueError):
            b.evaluate(X, data, labels, logits=logits)
