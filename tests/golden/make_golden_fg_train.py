#!/usr/bin/env python
"""Golden fixture for fg training, produced by the REFERENCE itself (build container only).

    python tests/golden/make_golden_fg_train.py

The reference ``FGModel`` (models/fg/fg_model.py), built as in make_golden_fgnet.py and filled with the counter-based weights
of tests/fg_ref64.py, runs its own ``loss()`` and ``loss.mean().backward()`` on the counter-based training batch of
tests/fg_train_ref.py (``make_batch(0, [3, 2])``: 5 instances, 3 in / 3 out, holes in feat_masks, bbox_masks and the label
depth_masks), once converted with ``.double()`` and once in fp32.  Neither weights nor inputs are stored.

g11_fgtrain.npz holds
  keys                         the state_dict key list
  none_keys                    the keys whose gradient is None (the mask head and the normalisation tensors)
  loss64_<name> / loss_err32_<name>   the seven [N] loss vectors in float64, and the fp32 run's max distance from them
  gmax_<i> / gerr32_<i>        per trained tensor (i = its state_dict position): max|g64|, the fp32 run's max|g32 - g64|
  g64_<i>                      g64 in full (tensors of at most 4096 elements), or
  gval_<i>                     g64 at fg_train_ref.sample_index(i, numel) (larger tensors: 4096 seeded samples; storing every
                               tensor in full would take 2.6 MB)
  sgd_loss64 / sgd_err32       [3, 7, N] / [3, 7]: the loss vectors of three SGD steps (lr 1e-3, no momentum,
                               clip_grad_norm_ 5.0 over model.parameters()) in float64, the fp32 run's distance per step
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import  # noqa: E402
import fg_ref64 as R  # noqa: E402
import fg_train_ref as T  # noqa: E402

_ref_import.install()
m = types.ModuleType('panoptic_forecasting.models.fg')
m.__path__ = [os.path.join(_ref_import.REF_ROOT, 'panoptic_forecasting', 'models', 'fg')]
sys.modules.setdefault('panoptic_forecasting.models.fg', m)
from panoptic_forecasting.models.fg.fg_model import FGModel  # noqa: E402

COUNTS = [3, 2]


def cast(d, dt):
    # fresh dicts per call: the reference's loss adds keys to the ones it is given
    return {k: (v.to(dt) if v.is_floating_point() else v.clone()) for k, v in d.items()}


def main():
    torch.set_grad_enabled(True)
    params = R.fg_params()
    params['use_bbox_ulbr'] = False
    model = FGModel(params).train()
    model.load_state_dict(R.fill_weights(model.state_dict()))
    inputs, labels = T.make_batch(0, COUNTS)
    keys = list(model.state_dict().keys())
    arrs = {'keys': np.array(keys)}
    runs = {}
    for dt in (torch.float64, torch.float32):
        mm = copy.deepcopy(model).to(dt)
        out = mm.loss(cast(inputs, dt), cast(labels, dt))
        assert tuple(out.keys()) == T.LOSS_KEYS, list(out.keys())
        out['loss'].mean().backward()
        runs[dt] = ({k: v.detach().double() for k, v in out.items()},
                    {k: (None if p.grad is None else p.grad.double()) for k, p in mm.named_parameters()})
    l64, g64 = runs[torch.float64]
    l32, g32 = runs[torch.float32]
    mine, mine_g = T.loss_and_grads(model.state_dict(), inputs, labels)
    for k in T.LOSS_KEYS:
        arrs['loss64_' + k] = l64[k].numpy()
        arrs['loss_err32_' + k] = np.float64((l32[k] - l64[k]).abs().max())
        print('%-20s fp32 err %.3e  checker err %.3e  max %.4g' % (k, arrs['loss_err32_' + k],
                                                                 (mine[k] - l64[k]).abs().max(), l64[k].abs().max()))
    none = [k for k in keys if g64[k] is None]
    assert none == [k for k in keys if not T.is_trained(k)], none
    arrs['none_keys'] = np.array(none)
    for i, k in enumerate(keys):
        if g64[k] is None:
            continue
        g = g64[k].numpy().reshape(-1)
        arrs['gmax_%d' % i] = np.float64(np.abs(g).max())
        arrs['gerr32_%d' % i] = np.float64((g32[k] - g64[k]).abs().max())
        if g.size <= T.SAMPLES:
            arrs['g64_%d' % i] = g
        else:
            arrs['gval_%d' % i] = g[T.sample_index(i, g.size)]
        print('%-45s max|g| %.3e  fp32 err/max %.2e  checker err/max %.2e  nonzero %.3f' % (
            k, arrs['gmax_%d' % i], arrs['gerr32_%d' % i] / arrs['gmax_%d' % i],
            (mine_g[k] - g64[k]).abs().max() / arrs['gmax_%d' % i], (g != 0).mean()))
    steps = {}
    for dt in (torch.float64, torch.float32):
        mm = copy.deepcopy(model).to(dt)
        opt = torch.optim.SGD([p for p in mm.parameters() if p.requires_grad], lr=1e-3)
        rows = []
        for _ in range(3):
            opt.zero_grad()
            out = mm.loss(cast(inputs, dt), cast(labels, dt))
            out['loss'].mean().backward()
            torch.nn.utils.clip_grad_norm_(mm.parameters(), 5.0)
            opt.step()
            rows.append(torch.stack([out[k].detach().double() for k in T.LOSS_KEYS]))
        steps[dt] = torch.stack(rows)
    arrs['sgd_loss64'] = steps[torch.float64].numpy()
    arrs['sgd_err32'] = (steps[torch.float32] - steps[torch.float64]).abs().amax(-1).numpy()
    print('sgd loss.mean per step', steps[torch.float64][:, -1].mean(-1).tolist())
    print('sgd fp32 err', arrs['sgd_err32'][:, -1].tolist())
    path = os.path.join(HERE, 'g11_fgtrain.npz')
    np.savez_compressed(path, **arrs)
    print('g11_fgtrain.npz', os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
