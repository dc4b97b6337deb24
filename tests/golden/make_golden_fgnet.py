#!/usr/bin/env python
"""Golden fixtures for the fg forecaster network, produced by the REFERENCE itself (build container only).

    python tests/golden/make_golden_fgnet.py

The reference ``FGModel`` (/root/reference/panoptic_forecasting/models/fg/fg_model.py) is built from the shipped fg config
(pretrained_models/fg/config.yaml) with non-zero normalisation parameters, filled with the counter-based weights of
tests/fg_ref64.py (``fill_weights``: uniform, scaled by fan-in; the predictor x40 so that the mask logits span several
units), and run unmodified on counter-based inputs (``make_inputs``): 2 images with 3 + 2 instances, instance 1 missing
at its first input step and without depth at its second, instance 3 missing at the most recent step, mixed output_inds.
Neither weights (89 MB) nor inputs are stored: the tests rebuild them bit for bit.

g8_fgnet.npz holds
  keys / shapes            the state_dict key list and shapes
  <out>64                  forward in float64 (model.double()): trajectories and masks, in full
  <out>_err32              the fp32 reference's own max |fp32 - fp64| per output tensor
  <out>_idx / _val         seeded samples (4096 values, float64) of mask_feats and output_feats, with <out>_maxabs
  seg_pan_fg / seg_pan_z_fg  predict_panoptic at 1024 x 2048 over a background with things >= 11 (use_depth_sorting off / on)
  seg_sem_fg               predict_semantics over the same background
The maps are stored as uint16 overlays: the pixels where the result differs from what the call gives without instances
(the background ``fg_ref64.background(1, 2)``, things set to 255 for predict_panoptic), 0 elsewhere; ``fg_ref64.seg_from_overlay``
rebuilds the full map exactly.  That keeps the file small: every full-size array would be a few hundred KB.
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import  # noqa: E402
import fg_ref64 as R  # noqa: E402

_ref_import.install()
m = types.ModuleType('panoptic_forecasting.models.fg')
m.__path__ = [os.path.join(_ref_import.REF_ROOT, 'panoptic_forecasting', 'models', 'fg')]
sys.modules.setdefault('panoptic_forecasting.models.fg', m)
from panoptic_forecasting.models.fg.fg_model import FGModel  # noqa: E402

torch.set_grad_enabled(False)
COUNTS = [3, 2]
OUTS = ('normalized_trajectory', 'unnormalized_trajectory', 'mask_feats', 'output_feats', 'masks')


def build(depth_sorting=False):
    params = R.fg_params()
    params['use_bbox_ulbr'] = False
    model = FGModel(params).eval()
    model.load_state_dict(R.fill_weights(model.state_dict()))
    model.use_depth_sorting = depth_sorting
    return model


def main():
    model = build()
    inputs, labels = R.make_inputs(0, COUNTS)
    args = R.forward_args(inputs, labels)
    out32 = model(*args)
    m64 = copy.deepcopy(model).double()
    a64 = tuple(a.double() if torch.is_tensor(a) and a.is_floating_point() else a for a in args)
    out64 = m64(*a64)
    mine = R.forward64(model.state_dict(), *args)
    arrs = {'keys': np.array(list(model.state_dict().keys())),
            'shapes': np.array([str(tuple(v.shape)) for v in model.state_dict().values()]),
            'counts': np.array(COUNTS, np.int32)}
    for k in OUTS:
        arrs[k + '_err32'] = np.float64((out32[k].double() - out64[k]).abs().max())
        print('%-24s fp32 err %.3e   checker err %.3e   max|x| %.3g' % (
            k, arrs[k + '_err32'], (mine[k] - out64[k]).abs().max(), out64[k].abs().max()))
    arrs['normalized_trajectory64'] = out64['normalized_trajectory'].numpy()
    arrs['unnormalized_trajectory64'] = out64['unnormalized_trajectory'].numpy()
    arrs['masks64'] = out64['masks'].numpy()
    rng = np.random.RandomState(8)
    for k in ('mask_feats', 'output_feats'):
        v = out64[k].numpy()
        idx = rng.choice(v.size, 4096, replace=False)
        arrs[k + '_idx'] = idx.astype(np.int64)
        arrs[k + '_val'] = v.reshape(-1)[idx]
        arrs[k + '_maxabs'] = np.float64(np.abs(v).max())
    lg = out64['masks']
    print('mask logits: min %.2f max %.2f frac>0 %.3f' % (lg.min(), lg.max(), (lg > 0).double().mean()))

    bg = R.background(1, len(COUNTS))
    inputs['background'] = [x.clone() for x in bg]
    arrs['seg_pan'] = model.predict_panoptic(inputs, labels)['seg'].numpy().astype(np.int32)
    inputs['background'] = [x.clone() for x in bg]
    arrs['seg_sem'] = model.predict_semantics(inputs, labels)['seg'].numpy().astype(np.int32)
    inputs['background'] = [x.clone() for x in bg]
    arrs['seg_pan_z'] = build(True).predict_panoptic(inputs, labels)['seg'].numpy().astype(np.int32)
    for k, panoptic in (('seg_pan', True), ('seg_sem', False), ('seg_pan_z', True)):
        seg = arrs.pop(k)
        v, c = np.unique(seg, return_counts=True)
        print(k, dict(zip(v.tolist(), c.tolist())))
        arrs[k + '_fg'] = R.seg_overlay(seg, bg.numpy(), panoptic)
        assert np.array_equal(R.seg_from_overlay(arrs[k + '_fg'], bg.numpy(), panoptic), seg)
    path = os.path.join(HERE, 'g8_fgnet.npz')
    np.savez_compressed(path, **arrs)
    print('g8_fgnet.npz', os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
