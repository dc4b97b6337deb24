#!/usr/bin/env python
"""Golden fixture G13 for the native fg scene dataset, produced by the REFERENCE's ``FGSceneDataset`` (build container only).

    python tests/golden/make_golden_fgscene.py

A tiny synthetic tree in the reference's formats (pickled frames through the real pandas; background PNGs through the real PIL) is
written into a temporary directory and the reference's own ``FGSceneDataset(split, params, test=True)`` and ``collate_fn``
(data/datasets/fg_scene_dataset.py) run on it, unmodified.  Stubs, in the style of _ref_import.py: ``cv2`` (imported by
``data_utils``, never used here) and ``h5py``, which is not installed: a dict-backed ``File`` whose datasets are numpy arrays (the
two reads the dataset makes are ``dset[list_of_rows]`` and ``dset[:]``).  Only data is recorded.

g13_fgscene.npz holds
  configs                         JSON: [{name, data: {...}, use_bbox_ulbr}] - the keys each configuration sets (paths excluded)
  scenes                          JSON: [[city, seq, frame], ...] (four scenes; the third keeps no instance under any configuration)
  in.meta.<col>.<i>               the columns feat_mask [n,30] bool, feat_ind [n,30] i64, track_id [n], class [n], bboxes [n,30,4] f64
  in.depth.<i>, in.cascade.<i>    depth [n,30] f64 of {split}_depth_seq_info / {split}_cascadedepth_seq_info
  in.condensed.<i>                feat_ind [n,30] of {split}_seq_condensed_feat_info
  in.feats.<i>, in.cfeats.<i>     the scene's feature dataset of {split}_feats.h5 / {split}_condensed_feats.h5 [rows <= 4,256,14,14] f32
  in.odometry.<i> [30,5], in.times.<i> [30]      {split}_3d_info
  in.odom_pred.<key>              the predicted-odometry export, '{city}/{seq}/{frame}/{start}' -> [9,2] ('/' written as '|')
  in.background.<i>               [16,32] u8 label map of the scene's target frame
  out.<config>.inputs.<key>.<i>, out.<config>.labels.<key>.<i>, out.<config>.meta.<key>.<i>
                                  what collate_fn returned for the four scenes as one batch (labels.feats left out: the native
                                  dataset does not produce it)
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import REF_ROOT  # noqa: E402

SPLIT = 'val'
SCENES = [('ulm', '000001', 19), ('ulm', '000002', 25), ('bonn', '000003', 19), ('bonn', '000004', 30)]
COUNTS = [5, 3, 2, 4]
MID = [4, 7, 10, 13, 16, 19]
SHORT = [10, 13, 16, 19, 22, 25]
BASE = {'require_most_recent': True, 'use_cascade_depths': True, 'use_condensed_feats': True, 'use_3d_info': True, 'no_feats': False}
CONFIGS = [
    {'name': 'mid', 'data': dict(BASE), 'use_bbox_ulbr': False, 'odom_pred': True, 'background': True},
    {'name': 'short', 'data': dict(BASE, output_ind=0), 'use_bbox_ulbr': False, 'odom_pred': True, 'background': True},
    {'name': 'gap', 'data': dict(BASE, filter_car_gap=20, max_depth=200), 'use_bbox_ulbr': False, 'odom_pred': True, 'background': True},
    {'name': 'gap_short', 'data': dict(BASE, filter_car_gap=20, max_depth=200, output_ind=0), 'use_bbox_ulbr': False, 'odom_pred': True,
     'background': True},
    {'name': 'ulbr', 'data': {'require_most_recent': False, 'use_condensed_feats': False, 'use_3d_info': True, 'filter_car_gap': 20,
                              'output_ind': 1}, 'use_bbox_ulbr': True, 'odom_pred': False, 'background': False},
]
H5_STORE = {}


class StubH5File:
    def __init__(self, path, mode='r'):
        self.d = H5_STORE[path]

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def __getitem__(self, name):
        return self.d[name]


def install_stubs():
    for name, path in (('panoptic_forecasting', REF_ROOT + '/panoptic_forecasting'),
                       ('panoptic_forecasting.data', REF_ROOT + '/panoptic_forecasting/data'),
                       ('panoptic_forecasting.data.datasets', REF_ROOT + '/panoptic_forecasting/data/datasets')):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = [path]
            sys.modules[name] = m
    if 'cv2' not in sys.modules:
        sys.modules['cv2'] = types.ModuleType('cv2')
    h5 = types.ModuleType('h5py')
    h5.File = StubH5File
    sys.modules['h5py'] = h5
    if not hasattr(np, 'float'):
        np.float = float
    sys.dont_write_bytecode = True  # the reference tree is read-only


def feature_rows(first_row, rows):
    """Small integer-valued planes: constant per channel but for one element whose place moves with the channel."""
    out = np.empty((rows, 256, 196), np.float32)
    for r in range(rows):
        base = ((first_row + r) * 37 + np.arange(256)) % 23
        out[r] = base[:, None]
        out[r, np.arange(256), (np.arange(256) + first_row + r) % 196] += 1
    return out.reshape(rows, 256, 14, 14)


def make_tables():
    g = np.random.RandomState(13)
    t = {'meta': [], 'depth': [], 'cascade': [], 'condensed': [], 'feats': [], 'cfeats': [], 'odometry': [], 'times': [], 'background': []}
    row0 = 0
    for i, n in enumerate(COUNTS):
        x0 = g.uniform(0, 1700, (n, 1)) + np.cumsum(g.uniform(-12, 12, (n, 30)), 1)
        y0 = g.uniform(200, 700, (n, 1)) + np.cumsum(g.uniform(-4, 4, (n, 30)), 1)
        w, h = g.uniform(20, 300, (n, 1)) + np.cumsum(g.uniform(-3, 3, (n, 30)), 1), g.uniform(20, 200, (n, 1)) + g.uniform(-3, 3, (n, 30))
        bboxes = np.stack([x0, y0, x0 + w, y0 + h], -1)
        mask = g.rand(n, 30) < 0.8
        mask[:, 10] = True
        mask[:, 16] = True
        cls = g.randint(11, 19, n)
        depth = g.uniform(5, 150, (n, 30))
        cascade = depth + g.uniform(-2, 2, (n, 30))
        if i == 0:
            # a car whose centre is left of the gap and whose WIDTH jumps: trips _filter_car_gap in its default (cwh) reading at frame 10
            # (mid) / 16 (short); its right edge jumps with it, so the ulbr reading trips too.  Frame 7 is unobserved.
            cls[0] = 13
            widths = {4: 40, 7: 50, 10: 80, 13: 85, 16: 150, 19: 155, 22: 160, 25: 165}
            for fr in range(30):
                wv = widths[max(k for k in widths if k <= max(fr, 4))]
                bboxes[0, fr] = [10 - wv / 2, 300, 10 + wv / 2, 400 + fr]
            mask[0] = True
            mask[0, 7] = False
            # a car at the right border whose LEFT edge jumps back: trips only the ulbr reading (found_x1)
            cls[1] = 13
            lefts = {4: 1900, 7: 1895, 10: 1850, 13: 1845, 16: 1800, 19: 1795, 22: 1790, 25: 1700}
            for fr in range(30):
                lv = lefts[max(k for k in lefts if k <= max(fr, 4))]
                bboxes[1, fr] = [lv, 500, 2040, 620]
            mask[1] = True
            cls[2] = 13                   # a car nowhere near a border: the filter leaves it alone
            for arr in (depth, cascade):
                arr[0, 4], arr[0, 13], arr[1, 10], arr[1, 16], arr[2, 7], arr[3, 19], arr[3, 22] = -1, 1000000, 250.5, -1, 1000000, 200, 200.5
            mask[3, 10], mask[3, 16], mask[3, 4] = False, False, True      # kept only without require_most_recent
            mask[4, 4], mask[4, 7] = False, False
        if i == 1:
            mask[0, 13:] = False
            for arr in (depth, cascade):
                arr[1, :] = -1
                arr[2, 10:20] = 300
        if i == 2:
            mask[:, :17] = False          # nothing observed at any input step of either window: zero instances kept
        if i == 3:
            cls[0] = 13
            bboxes[0, :, 0], bboxes[0, :, 2] = 5, 5 + np.arange(30) * 9.5       # left edge inside the gap, width grows 28.5 a step
        rows = [4, 4, 2, 3][i]
        ind = np.where(mask, g.randint(0, rows, (n, 30)), -1)
        cond = np.where(mask, g.randint(0, rows, (n, 30)), -1)
        if i == 0:
            ind[2, 10], cond[2, 10], cond[0, 4] = -1, -1, -1        # observed, but no feature row
        t['meta'].append({'feat_mask': mask, 'feat_ind': ind.astype(np.int64), 'track_id': np.arange(n) + 100 * (i + 1), 'class': cls.astype(np.int64),
                          'bboxes': bboxes})
        t['depth'].append(depth)
        t['cascade'].append(cascade)
        t['condensed'].append(cond.astype(np.int64))
        t['feats'].append(feature_rows(row0, rows))
        t['cfeats'].append(feature_rows(row0 + 50, rows))
        row0 += rows
        odom = g.uniform(-1, 1, (30, 5)) * [3, 0.05, 0.2, 0.02, 0.01] + [8, 0, 0.45, 0, 0]
        t['odometry'].append(odom)
        t['times'].append(1000.0 * (i + 1) + np.cumsum(g.uniform(0.055, 0.062, 30)))
        bg = g.randint(0, 19, (16, 32)).astype(np.uint8)
        bg[g.rand(16, 32) < 0.1] = 255
        t['background'].append(bg)
    t['odom_pred'] = {}
    for (city, seq, frame) in SCENES:
        for start in (MID[2], SHORT[2]):
            pred = g.uniform(-1, 1, (9, 2)) * [3, 0.05] + [8, 0]
            pred[4, 1] = 1e-5          # below the straight-line threshold of get_vehicle_now_T_prev
            t['odom_pred']['%s/%s/%d/%d' % (city, seq, frame, start)] = pred.astype(np.float32)
    return t


def write_tree(root, t):
    import pandas as pd
    ident = {'city': [s[0] for s in SCENES], 'seq': [s[1] for s in SCENES], 'frame': [s[2] for s in SCENES]}
    frame = lambda cols: pd.DataFrame(dict(ident, **cols))     # noqa: E731
    frame({k: [m[k] for m in t['meta']] for k in t['meta'][0]}).to_pickle(os.path.join(root, '%s_seq_meta.pkl' % SPLIT))
    frame({'depth': t['depth']}).to_pickle(os.path.join(root, '%s_depth_seq_info.pkl' % SPLIT))
    frame({'depth': t['cascade']}).to_pickle(os.path.join(root, '%s_cascadedepth_seq_info.pkl' % SPLIT))
    frame({'feat_ind': t['condensed']}).to_pickle(os.path.join(root, '%s_seq_condensed_feat_info.pkl' % SPLIT))
    frame({'odometry': t['odometry'], 'times': t['times']}).to_pickle(os.path.join(root, '%s_3d_info.pkl' % SPLIT))
    name = lambda s: '%s/%s/%d' % s                             # noqa: E731
    H5_STORE[os.path.join(root, '%s_feats.h5' % SPLIT)] = {name(s): t['feats'][i] for i, s in enumerate(SCENES)}
    open(os.path.join(root, '%s_feats.h5' % SPLIT), 'w').close()          # the reference tests the path's existence (:76)
    H5_STORE[os.path.join(root, '%s_condensed_feats.h5' % SPLIT)] = {name(s): t['cfeats'][i] for i, s in enumerate(SCENES)}
    H5_STORE[os.path.join(root, 'odom', 'predicted_odometry_%s.h5' % SPLIT)] = t['odom_pred']
    for i, (city, seq, fr) in enumerate(SCENES):
        d = os.path.join(root, 'bg', SPLIT, city)
        os.makedirs(d, exist_ok=True)
        Image.fromarray(t['background'][i]).save(os.path.join(d, '%s_%s_%06d_gtFine_labelIds.png' % (city, seq, fr)))


def params_for(cfg, root):
    data = dict(cfg['data'], data_dir=root, depth_dir=root, feats_dir=root, info_3d_dir=root, data_splits=[SPLIT])
    if cfg['odom_pred']:
        data['odom_pred_dir'] = os.path.join(root, 'odom')
    if cfg['background']:
        data['background_dir'] = os.path.join(root, 'bg')
    return {'data': data, 'use_bbox_ulbr': cfg['use_bbox_ulbr']}


def main():
    install_stubs()
    from panoptic_forecasting.data.datasets import fg_scene_dataset as ref
    t = make_tables()
    arrs = {'configs': np.array(json.dumps(CONFIGS)), 'scenes': np.array(json.dumps(SCENES))}
    for i in range(len(SCENES)):
        for col, v in t['meta'][i].items():
            arrs['in.meta.%s.%d' % (col, i)] = v
        for k in ('depth', 'cascade', 'condensed', 'feats', 'cfeats', 'odometry', 'times', 'background'):
            arrs['in.%s.%d' % (k, i)] = t[k][i]
    for k, v in t['odom_pred'].items():
        arrs['in.odom_pred.' + k.replace('/', '|')] = v
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, t)
        for cfg in CONFIGS:
            params = params_for(cfg, root)
            ds = ref.FGSceneDataset(SPLIT, params, test=True)
            assert len(ds) == len(SCENES) and params['data']['num_classes'] == 19 and params['data']['odom_size'] == 5
            batch = ref.collate_fn([ds[i] for i in range(len(ds))])
            kept = [len(x) for x in batch['inputs']['classes']]
            print('%-10s kept %s target %s' % (cfg['name'], kept, batch['meta']['target_frame']))
            assert kept[2] == 0 and max(kept) <= 5
            for group in ('inputs', 'labels', 'meta'):
                for key, vals in batch[group].items():
                    if group == 'labels' and key == 'feats':
                        continue
                    for i, v in enumerate(vals):
                        v = v.numpy() if torch.is_tensor(v) else np.asarray(v)
                        arrs['out.%s.%s.%s.%d' % (cfg['name'], group, key, i)] = v
            if cfg['name'] in ('gap', 'ulbr'):           # the filter fired: some step of a class-13 track is zeroed
                raw = ref.FGSceneDataset(SPLIT, params_for(dict(cfg, data={k: v for k, v in cfg['data'].items() if k != 'filter_car_gap'}),
                                                           root), test=True)[0]['inputs']['bbox_masks']
                assert not torch.equal(raw, batch['inputs']['bbox_masks'][0]), cfg['name']
    out = os.path.join(HERE, 'g13_fgscene.npz')
    np.savez_compressed(out, **arrs)
    print('wrote %s (%d bytes)' % (out, os.path.getsize(out)))


if __name__ == '__main__':
    main()
