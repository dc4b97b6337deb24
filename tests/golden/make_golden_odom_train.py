#!/usr/bin/env python
"""Golden fixture for odom training, produced by the REFERENCE itself (build container only).

    python tests/golden/make_golden_odom_train.py

The reference's ``OdomDataset('train', test=False)`` (data/datasets/odom_dataset.py) runs unmodified over the synthetic
snippets of make_golden_odomnet.py written as ``train_3d_info.pkl``: its items are the training windows, and the
``odom_norm_params`` it leaves in ``params['data']`` the normalisation of the train split.  The reference ``OdomModel``
(models/odom/odom_model.py), filled with the counter-based weights of tests/odom_ref64.py and converted with
``.double()``, runs its own ``loss()`` on counter-based inputs and labels (B = 32, 9 in / 9 out) in two configurations;
``loss.mean().backward()`` gives the gradients of the six trainable tensors.  Stubs as in make_golden_odomnet.py.

g10_odomtrain.npz holds
  snip_odometry                       the synthetic train_3d_info.pkl (3 snippets, odometry [30, 5] float64)
  win_inputs / win_labels / win_start the training dataset's items, in order (15 per snippet)
  norm_mean / norm_std                odom_norm_params (float32 [2])
  <cfg>_loss64                        loss()['loss'] in float64, cfg a = direct / mse / normalised, b = offset / smooth_l1 /
                                      unnormalised (odom_train_ref.CONFIGS)
  <cfg>_grad_<key>                    d loss.mean() / d key in float64 for the six trainable tensors
"""
import copy
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_odomnet as G  # noqa: E402  (installs the reference import hook)
import odom_ref64 as R  # noqa: E402
import odom_train_ref as T  # noqa: E402


def main():
    import pandas as pd
    torch.set_grad_enabled(True)
    G.install_stubs()
    from panoptic_forecasting.data.datasets.odom_dataset import OdomDataset
    from panoptic_forecasting.models.odom.odom_model import OdomModel
    arrs = {}
    names, odo = G.snippets()
    tmp = tempfile.mkdtemp()
    pd.DataFrame({'city': [n[0] for n in names], 'seq': [n[1] for n in names], 'frame': [n[2] for n in names],
                  'odometry': list(odo)}).to_pickle(os.path.join(tmp, 'train_3d_info.pkl'))
    arrs['snip_odometry'] = odo
    params = {'data': {'data_dir': tmp}}
    ds = OdomDataset('train', params, test=False)
    items = [ds[i] for i in range(len(ds))]
    arrs['win_inputs'] = np.stack([it['inputs']['odometry'].numpy() for it in items])
    arrs['win_labels'] = np.stack([it['labels']['odometry'].numpy() for it in items])
    arrs['win_start'] = np.array([int(it['meta']['start_frame']) for it in items], np.int64)
    mean, std = params['data']['odom_norm_params']
    arrs['norm_mean'], arrs['norm_std'] = mean.numpy(), std.numpy()
    print('%d training windows, norm mean %s std %s' % (len(items), mean.tolist(), std.tolist()))
    inps, labels = R.make_inputs(0, 32), T.make_labels(0, 32)
    for cfg, mode, loss_fn, normalised in T.CONFIGS:
        model = OdomModel(R.odom_params(predict_type=mode, loss_fn=loss_fn, use_normalized_loss=normalised))
        model.load_state_dict(R.fill_weights(model.state_dict()))
        m64 = copy.deepcopy(model).double()
        loss = m64.loss({'odometry': inps.double()}, {'odometry': labels.double()})['loss']
        loss.mean().backward()
        arrs[cfg + '_loss64'] = loss.detach().numpy()
        sd = dict(m64.named_parameters())
        for k in T.TRAINABLE:
            arrs[cfg + '_grad_' + k] = sd[k].grad.numpy()
        mine, grads = T.loss_and_grads(model.state_dict(), inps, labels, mode, loss_fn, normalised)
        err = max(((grads[k] - sd[k].grad).abs().max() / sd[k].grad.abs().max()).item() for k in T.TRAINABLE)
        print('%s %-6s %-9s normalised=%s  loss %.4f  checker: loss err %.2e  grad err %.2e (rel)' % (
            cfg, mode, loss_fn, normalised, loss.mean().item(), (mine - loss.detach()).abs().max().item(), err))
    path = os.path.join(HERE, 'g10_odomtrain.npz')
    np.savez_compressed(path, **arrs)
    print('g10_odomtrain.npz', os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
