"""Test helper for odom training (not a test module): the reference's loss lines (odom_model.py:104-115) on top of
``odom_ref64.forward64``, and its gradients by autograd in float64 (the checker) or float32 (the yardstick of the
gradient bar).  tests/test_odom_train_host.py pins it to the reference's own float64 run in g10_odomtrain.npz.
"""
import torch
import torch.nn.functional as F

import odom_ref64 as R

TRAINABLE = ('rnn.weight_ih_l0', 'rnn.weight_hh_l0', 'rnn.bias_ih_l0', 'rnn.bias_hh_l0', 'out.0.weight', 'out.0.bias')
# (name, predict_type, loss_fn, use_normalized_loss): the fixture's two configurations
CONFIGS = (('a', 'direct', 'mse', True), ('b', 'offset', 'smooth_l1', False))


def loss_ref(sd, inps, labels, predict_type='direct', loss_fn='mse', normalised=True, dtype=torch.float64):
    """OdomModel.loss of the shipped config in ``dtype``: the per-sequence losses [B]."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    preds, norm = R.forward64(sd, inps, labels.shape[1], predict_type, dtype)
    labels = labels.to(dtype)
    fn = F.smooth_l1_loss if loss_fn == 'smooth_l1' else F.mse_loss
    if normalised:
        loss = fn(norm, (labels - sd['odom_mean']) / sd['odom_std'], reduction='none')
    else:
        loss = fn(preds, labels, reduction='none')
    return loss.reshape(loss.shape[0], -1).mean(1)


def loss_and_grads(sd, inps, labels, predict_type='direct', loss_fn='mse', normalised=True, dtype=torch.float64, weights=None):
    """(losses [B], {key: d(sum_b weights_b * loss_b) / d key}) in ``dtype`` (weights default to 1/B: the training mean)."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(k in TRAINABLE) for k, v in sd.items()}
    loss = loss_ref(leaves, inps, labels, predict_type, loss_fn, normalised, dtype)
    scalar = loss.mean() if weights is None else (loss * weights.to(loss)).sum()
    grads = torch.autograd.grad(scalar, [leaves[k] for k in TRAINABLE])
    return loss.detach(), dict(zip(TRAINABLE, grads))


def make_labels(case, b, t_out=9):
    """[b, t_out, 2] float32 labels: the input generator's stream family, input numbers 2 and 3."""
    import numpy as np
    from fg_ref64 import uniform
    u = lambda j: torch.from_numpy(uniform(2000 + 100 * case + j, b * t_out).astype(np.float32).reshape(b, t_out))
    return torch.stack([14 * u(2), 0.3 * (u(3) - 0.5)], -1)
