#!/usr/bin/env python
"""Golden fixtures for the odometry forecaster, produced by the REFERENCE itself (build container only).

    python tests/golden/make_golden_odomnet.py

The reference ``OdomModel`` (models/odom/odom_model.py) is built from the shipped odom config
(pretrained_models/odom/config.yaml) with non-zero normalisation parameters, filled with the counter-based weights of
tests/odom_ref64.py (``fill_weights``) and run unmodified on counter-based inputs (``make_inputs``: B = 32, T_in = 9,
T_out = 9).  Its ``OdomDataset(test=True)`` (data/datasets/odom_dataset.py) and its export's ``export_results``
(experiments/export_cityscapes_odom.py) run unmodified over a small synthetic ``val_3d_info.pkl`` written to a temp
folder; h5py and torchvision are absent here, so ``h5py.File`` is a stand-in that records what ``create_dataset`` is
handed, and ``torchvision.transforms`` an empty module (``load_imgs`` is off).  The export's other imports (dataset and
model builders, misc, train_utils, config) are only used by its ``__main__`` block and are stubbed.

g9_odomnet.npz holds
  keys / shapes                  the state_dict key list and shapes
  <mode>_out64 / _norm64         forward in float64 (model.double()) for predict_type direct and offset
  <mode>_out_err32 / _norm_err32 the fp32 reference's own max |fp32 - fp64| per output
  snip_city / _seq / _frame / _odometry   the synthetic val_3d_info.pkl (3 snippets, odometry [30, 5] float64)
  win_inputs / win_labels / win_city / win_seq / win_frame / win_start   the dataset's items, in order
  export_names / export_data     the (name, data) pairs export_results hands to create_dataset, in order (direct)
  export64 / export_err32        the same windows through the float64 model, and the fp32 export's max error
  fgo_inp_odom / fgo_preds / fgo_times / fgo_rows   fg_odometry cases through data_utils.get_vehicle_now_T_prev
"""
import copy
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import  # noqa: E402
import odom_ref64 as R  # noqa: E402

_ref_import.install()
REF = _ref_import.REF_ROOT
torch.set_grad_enabled(False)
CREATED = []      # (name, data) pairs handed to the h5py stand-in


class _File:
    def __init__(self, path, mode='r'):
        assert mode == 'w', mode

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def create_dataset(self, name, data):
        CREATED.append((name, np.array(data)))


def install_stubs():
    def module(name, path=None, **attrs):
        m = types.ModuleType(name)
        if path:
            m.__path__ = [os.path.join(REF, path)]
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    module('h5py', File=_File)
    tv = module('torchvision')
    tv.transforms = module('torchvision.transforms')
    module('panoptic_forecasting.data.datasets', 'panoptic_forecasting/data/datasets')
    module('panoptic_forecasting.models.odom', 'panoptic_forecasting/models/odom')
    # imported by the export script for its __main__ block only
    sys.modules['panoptic_forecasting.data'].build_dataset = None
    sys.modules['panoptic_forecasting.models'].build_model = None
    module('panoptic_forecasting.utils', 'panoptic_forecasting/utils')
    module('panoptic_forecasting.utils.misc')
    module('panoptic_forecasting.utils.config', load_config=None)
    module('panoptic_forecasting.training', 'panoptic_forecasting/training')
    module('panoptic_forecasting.training.train_utils')


def load_export_script():
    spec = importlib.util.spec_from_file_location('export_cityscapes_odom',
                                                  os.path.join(REF, 'panoptic_forecasting/experiments/export_cityscapes_odom.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(predict_type):
    from panoptic_forecasting.models.odom.odom_model import OdomModel
    model = OdomModel(R.odom_params(predict_type=predict_type)).eval()
    model.load_state_dict(R.fill_weights(model.state_dict()))
    return model


def snippets():
    """3 snippets: smooth speed / yaw-rate curves with noise, one with a straight stretch (|yaw| < 0.000175)."""
    rng = np.random.Generator(np.random.PCG64(91))
    names = [('aachen', '000003', 19), ('bonn', '000041', 33), ('ulm', '000007', 25)]
    odo = []
    for i in range(len(names)):
        t = np.arange(30)
        speed = 6 + 4 * np.sin(0.2 * t + i) + rng.normal(0, 0.3, 30)
        yaw = 0.08 * np.sin(0.15 * t + 2 * i) + rng.normal(0, 0.01, 30)
        if i == 2:
            yaw[10:20] = 1e-5
        rest = rng.normal(0, 1, (30, 3))
        odo.append(np.concatenate([np.stack([speed, yaw], 1), rest], 1))
    return names, np.stack(odo)


def main():
    import pandas as pd
    install_stubs()
    from panoptic_forecasting.data import data_utils
    from panoptic_forecasting.data.datasets.odom_dataset import OdomDataset, collate_fn
    export = load_export_script()
    arrs = {}
    # ---- the network
    inps = R.make_inputs(0, 32)
    for mode in ('direct', 'offset'):
        model = build(mode)
        if mode == 'direct':
            arrs['keys'] = np.array(list(model.state_dict().keys()))
            arrs['shapes'] = np.array([str(tuple(v.shape)) for v in model.state_dict().values()])
        out32, norm32 = model(inps, 9)
        m64 = copy.deepcopy(model).double()
        out64, norm64 = m64(inps.double(), 9)
        mine, mine_n = R.forward64(model.state_dict(), inps, 9, mode)
        arrs[mode + '_out64'], arrs[mode + '_norm64'] = out64.numpy(), norm64.numpy()
        arrs[mode + '_out_err32'] = np.float64((out32.double() - out64).abs().max())
        arrs[mode + '_norm_err32'] = np.float64((norm32.double() - norm64).abs().max())
        print('%-6s fp32 err %.3e / %.3e   checker err %.3e   max|x| %.3g' % (
            mode, arrs[mode + '_out_err32'], arrs[mode + '_norm_err32'], max((mine - out64).abs().max(), (mine_n - norm64).abs().max()),
            out64.abs().max()))
    # ---- the dataset's windows and the export over a synthetic val_3d_info.pkl
    names, odo = snippets()
    tmp = tempfile.mkdtemp()
    pd.DataFrame({'city': [n[0] for n in names], 'seq': [n[1] for n in names], 'frame': [n[2] for n in names],
                  'odometry': list(odo)}).to_pickle(os.path.join(tmp, 'val_3d_info.pkl'))
    arrs['snip_city'] = np.array([n[0] for n in names])
    arrs['snip_seq'] = np.array([n[1] for n in names])
    arrs['snip_frame'] = np.array([n[2] for n in names], np.int64)
    arrs['snip_odometry'] = odo
    params = {'data': {'data_dir': tmp}, 'no_gpu': True, 'working_dir': tmp, 'export_name': None,
              'training': {'batch_size': 32}}
    ds = OdomDataset('val', params, test=True)
    items = [ds[i] for i in range(len(ds))]
    arrs['win_inputs'] = np.stack([it['inputs']['odometry'].numpy() for it in items])
    arrs['win_labels'] = np.stack([it['labels']['odometry'].numpy() for it in items])
    for k in ('city', 'seq'):
        arrs['win_' + k] = np.array([it['meta'][k] for it in items])
    arrs['win_frame'] = np.array([int(it['meta']['frame']) for it in items], np.int64)
    arrs['win_start'] = np.array([int(it['meta']['start_frame']) for it in items], np.int64)
    model = build('direct')
    params['collate_fn'] = collate_fn
    export.export_results(model, ds, 'val', params)
    arrs['export_names'] = np.array([n for n, _ in CREATED])
    arrs['export_data'] = np.stack([d for _, d in CREATED]).astype(np.float32)
    out64, _ = copy.deepcopy(model).double()(torch.from_numpy(arrs['win_inputs']).double(), 9)
    arrs['export64'] = out64.numpy()
    arrs['export_err32'] = np.float64(np.abs(arrs['export_data'] - arrs['export64']).max())
    print('export: %d datasets, fp32 err %.3e' % (len(CREATED), arrs['export_err32']))
    # ---- fg odometry rows (fg_scene_dataset.py:476-492) from forecasts of the export, through the reference's motion model
    rng = np.random.Generator(np.random.PCG64(92))
    cases = []
    for c, idx in enumerate((0, 30, 60)):
        preds = arrs['export_data'][idx].copy()
        if c == 2:
            preds[5, 1] = np.float32(2e-5)                     # the straight-line branch (|yaw_rate| < 0.000175)
        times = 1.5e9 + np.cumsum(rng.uniform(0.055, 0.062, 7))
        inp_odom = rng.normal(0, 1, (3, 5))
        avg_delta_t = np.mean(times[1:] - times[:-1])
        final = []
        for speed, yaw_rate in preds:
            _, dx, dy, dtheta = data_utils.get_vehicle_now_T_prev(speed, yaw_rate, avg_delta_t)
            final.append(np.array([speed, yaw_rate, dx, dy, dtheta]))
        rows = torch.from_numpy(np.concatenate([inp_odom, np.stack(final)[[2, 5, 8]]])).float().numpy()
        cases.append((inp_odom, preds, times, rows))
    for j, k in enumerate(('fgo_inp_odom', 'fgo_preds', 'fgo_times', 'fgo_rows')):
        arrs[k] = np.stack([c[j] for c in cases])
    path = os.path.join(HERE, 'g9_odomnet.npz')
    np.savez_compressed(path, **arrs)
    print('g9_odomnet.npz', os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
