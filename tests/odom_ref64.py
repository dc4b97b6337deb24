"""Test helper for the odometry forecaster (not a test module): the shipped params, deterministic fills and a float64
functional checker.

Fills are counter-based (``fg_ref64.uniform``: the murmur3 finaliser over the element index, one stream per state_dict
key or per input), so the generator (tests/golden/make_golden_odomnet.py) and the tests rebuild the same weights and
inputs bit for bit without storing them.  Streams: the index of the state_dict key for the weights, 2000 + 100*case +
input number for the inputs.

``forward64`` restates OdomModel.forward (odom_model.py:79-106) in functional torch ops for the supported configuration;
tests/test_odom_host.py pins it to the reference's own float64 run in the fixture.
"""
import numpy as np
import torch

from fg_ref64 import sym, uniform

HID = 128
ODOM_MEAN = [5.5, 0.003]        # speed [m/s], yaw rate [rad/s]: Cityscapes-like scales
ODOM_STD = [4.0, 0.09]

ODOM_CONFIG = {'model_type': 'simple_odom', 'predict_type': 'direct', 'normalize_input': True, 'use_normalized_loss': True,
               'rnn_hidden': 128, 'loss_fn': 'mse'}      # pretrained_models/odom/config.yaml


def odom_params(**model_overrides):
    model = dict(ODOM_CONFIG)
    model.update(model_overrides)
    return {'task': 'odom', 'no_gpu': True, 'load_model': None, 'load_best_model': False, 'model': model,
            'data': {'odom_norm_params': [torch.tensor(ODOM_MEAN), torch.tensor(ODOM_STD)]}}


def fill_weights(state_dict):
    """The fixture's weights for a state_dict of the shipped shapes (keys in state_dict order = the streams)."""
    out = {}
    norms = {'odom_mean': ODOM_MEAN, 'odom_std': ODOM_STD}
    for s, (k, v) in enumerate(state_dict.items()):
        if k in norms:
            out[k] = torch.tensor(norms[k], dtype=torch.float32).reshape(v.shape)
        elif v.dim() == 1:
            out[k] = sym(s, tuple(v.shape), 0.1)
        else:
            out[k] = sym(s, tuple(v.shape), (3.0 / v.shape[1]) ** 0.5)
    return out


def make_inputs(case, b, t_in=9):
    """[b, t_in, 2] float32 unnormalised odometry: speed in [0, 14), yaw rate in [-0.15, 0.15); stream 2000 + 100*case."""
    u = lambda j: torch.from_numpy(uniform(2000 + 100 * case + j, b * t_in).astype(np.float32).reshape(b, t_in))
    return torch.stack([14 * u(0), 0.3 * (u(1) - 0.5)], -1)


def forward64(sd, inps, output_len, predict_type='direct', dtype=torch.float64):
    """OdomModel.forward of the shipped config in float64 (or ``dtype``): (results, normalized_results)."""
    d = dtype
    sd = {k: v.to(d) for k, v in sd.items()}
    mean, std = sd['odom_mean'], sd['odom_std']
    x = (inps.to(d) - mean) / std
    w_ih, w_hh = sd['rnn.weight_ih_l0'], sd['rnn.weight_hh_l0']
    b_ih, b_hh = sd['rnn.bias_ih_l0'], sd['rnn.bias_hh_l0']

    def gru(xt, h):
        ir, iz, inn = (xt @ w_ih.t() + b_ih).chunk(3, -1)
        hr, hz, hn = (h @ w_hh.t() + b_hh).chunk(3, -1)
        r = torch.sigmoid(ir + hr)
        z = torch.sigmoid(iz + hz)
        n = torch.tanh(inn + r * hn)
        return (1 - z) * n + z * h

    h = torch.zeros(x.shape[0], w_hh.shape[1], dtype=d, device=x.device)
    for t in range(x.shape[1] - 1):
        h = gru(x[:, t], h)
    cur = x[:, -1]
    res = []
    for _ in range(output_len):
        h = gru(cur, h)
        y = h @ sd['out.0.weight'].t() + sd['out.0.bias']
        cur = cur + y if predict_type == 'offset' else y
        res.append(cur)
    norm = torch.stack(res, 1)
    return norm * std + mean, norm
