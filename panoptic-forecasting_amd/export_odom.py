#!/usr/bin/env python
"""Export driver with the reference's flags - drop-in for ``experiments/export_cityscapes_odom.py``.

    python -u panoptic-forecasting_amd/export_odom.py --load_best_model --working_dir experiments/odom/

i.e. ``scripts/odom/export_odom.sh`` with the python path changed.
Same flags (``--export_name`` + the base set of ``utils/config.py``), same windows (``OdomDataset(test=True)``,
restated by ``odom_io.odom_windows``: 24 per snippet of ``{data.data_dir}/{split}_3d_info.pkl``), same keys
(``'%s/%s/%d/%d' % (city, seq, frame, start_frame)``, one ``[output_len, 2]`` float32 forecast each).  The file is
``<working_dir>/<export_name or 'odometry'>_<split>.npz``: the ``.npz`` twin that ``odom_io.OdometryFile`` opens when it is
given the reference's ``.h5`` name (there is no HDF5 writer here).  All windows of a split go through the model in one
``predict`` call.  ``data.use_orbslam_odom`` (ORB-SLAM odometry source) and ``data.load_imgs`` are refused.
"""
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if __package__ in (None, ''):                     # run as a script: make the package importable under its alias
    sys.path.insert(0, os.path.dirname(_HERE))
    import panoptic_forecasting_amd  # noqa: F401
    __package__ = 'panoptic_forecasting_amd'

from . import config as pfconfig   # noqa: E402
from . import odom_io              # noqa: E402
from .registry import build_model  # noqa: E402

EXTRA_FLAGS = (('--export_name', {}),)


def check_data(params):
    data = params.get('data', {})
    for key in ('use_orbslam_odom', 'load_imgs'):
        if data.get(key):
            raise ValueError('export_odom: data.%s is not supported (the 3d_info odometry windows are built)' % key)


def split_windows(data_dir, split, input_len=9, output_len=9):
    """(inputs [N,input_len,2], labels [N,output_len,2], keys [(city, seq, frame, start_frame)]) of every snippet, in the
    reference dataset's order."""
    import pandas as pd
    table = pd.read_pickle(os.path.join(data_dir, '%s_3d_info.pkl' % split))
    inputs, labels, keys = [], [], []
    for i in range(len(table)):
        row = table.iloc[i]
        inp, lab, starts = odom_io.odom_windows(row['odometry'], input_len, output_len)
        inputs.append(inp)
        labels.append(lab)
        keys += [(row['city'], row['seq'], int(row['frame']), int(s)) for s in starts]
    return np.concatenate(inputs), np.concatenate(labels), keys


def out_path(params, split):
    return os.path.join(params['working_dir'], '%s_%s.npz' % (params.get('export_name') or 'odometry', split))


def export_split(model, split, params):
    data = params['data']
    inputs, labels, keys = split_windows(data['data_dir'], split, data.get('input_len', 9), data.get('output_len', 9))
    dev = model.packed_weights().device
    with torch.no_grad():
        pred = model.predict({'odometry': torch.from_numpy(inputs).to(dev)}, {'odometry': torch.from_numpy(labels)})
    odom = pred['odometry'].cpu().numpy()
    path = out_path(params, split)
    odom_io.write_npz(path, dict(zip(keys, odom)))
    return path


def main(argv=None):
    params = pfconfig.load_config(EXTRA_FLAGS, argv)
    torch.manual_seed(params['seed'])
    check_data(params)
    model = build_model(params)
    model.eval()
    for split in params['data']['data_splits']:
        print('export_odom: wrote', export_split(model, split, params))


if __name__ == '__main__':
    main()
