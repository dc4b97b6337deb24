"""Test helper for the native fg scene dataset (not a test module): writes dataset trees into a temporary directory.

``write_g13`` lays the input tables recorded in tests/golden/g13_fgscene.npz out as files, either as the ``.npz`` twins or as the
reference's pickled frames (pandas; the H5 files always as twins: h5py is absent), and ``g13_params`` builds the params of one of
the fixture's configurations over such a tree.  ``write_synthetic`` writes a seeded twin tree of full-size scenes for the
end-to-end export test.
"""
import json
import os

import numpy as np
import torch

SPLIT = 'val'
META_COLS = ('feat_mask', 'feat_ind', 'track_id', 'class', 'bboxes')


def _table_arrays(ident, cols):
    """The twin's entries without pandas: the layout fg_dataset.frame_to_arrays documents."""
    out = {k: np.array(v) for k, v in ident.items()}
    for col, vals in cols.items():
        if len({v.shape for v in vals}) == 1:
            out[col] = np.stack(vals)
        else:
            out[col] = np.concatenate(vals)
            out[col + '__rows'] = np.array([len(v) for v in vals], np.int64)
    return out


def write_tables(root, scenes, tables, as_pkl=False):
    """``tables``: {'meta': {col: [per scene]}, 'depth': {file kind: [per scene]}, 'condensed': [...], 'feats': {file name: [per scene]},
    'odometry': [...], 'times': [...], 'odom_pred': {key: [9,2]}, 'background': {(scene index, target frame): [H,W] u8}}."""
    from panoptic_forecasting_amd import hop_io, odom_io
    os.makedirs(root, exist_ok=True)
    ident = {'city': [s[0] for s in scenes], 'seq': [s[1] for s in scenes], 'frame': [int(s[2]) for s in scenes]}

    def save(name, cols):
        path = os.path.join(root, name)
        if as_pkl:
            import pandas as pd
            pd.DataFrame(dict(ident, **{k: list(v) for k, v in cols.items()})).to_pickle(path)
        else:
            np.savez_compressed(os.path.splitext(path)[0] + '.npz', **_table_arrays(ident, cols))

    save('%s_seq_meta.pkl' % SPLIT, tables['meta'])
    for kind, vals in tables['depth'].items():
        save('%s_%s_seq_info.pkl' % (SPLIT, kind), {'depth': vals})
    if tables.get('condensed') is not None:
        save('%s_seq_condensed_feat_info.pkl' % SPLIT, {'feat_ind': tables['condensed']})
    if tables.get('odometry') is not None:
        save('%s_3d_info.pkl' % SPLIT, {'odometry': tables['odometry'], 'times': tables['times']})
    for fname, vals in tables['feats'].items():
        np.savez_compressed(os.path.join(root, os.path.splitext(fname)[0] + '.npz'),
                            **{'%s/%s/%d' % (s[0], s[1], int(s[2])): vals[i] for i, s in enumerate(scenes)})
    if tables.get('odom_pred'):
        os.makedirs(os.path.join(root, 'odom'), exist_ok=True)
        odom_io.write_npz(os.path.join(root, 'odom', 'predicted_odometry_%s.npz' % SPLIT),
                          {tuple(k.split('/')): v for k, v in tables['odom_pred'].items()})
    for (i, target), arr in tables.get('background', {}).items():
        city, seq = scenes[i][0], scenes[i][1]
        d = os.path.join(root, 'bg', SPLIT, city)
        os.makedirs(d, exist_ok=True)
        hop_io.write_png(os.path.join(d, hop_io.LABEL_PNG % (city, seq, target)), arr)


def g13_scenes(fx):
    return [tuple(s) for s in json.loads(str(fx['scenes']))]


def g13_configs(fx):
    return {c['name']: c for c in json.loads(str(fx['configs']))}


def write_g13(root, fx, as_pkl=False):
    scenes = g13_scenes(fx)
    n = range(len(scenes))
    tables = {'meta': {col: [fx['in.meta.%s.%d' % (col, i)] for i in n] for col in META_COLS},
              'depth': {'depth': [fx['in.depth.%d' % i] for i in n], 'cascadedepth': [fx['in.cascade.%d' % i] for i in n]},
              'condensed': [fx['in.condensed.%d' % i] for i in n],
              'feats': {'%s_feats.h5' % SPLIT: [fx['in.feats.%d' % i] for i in n],
                        '%s_condensed_feats.h5' % SPLIT: [fx['in.cfeats.%d' % i] for i in n]},
              'odometry': [fx['in.odometry.%d' % i] for i in n], 'times': [fx['in.times.%d' % i] for i in n],
              'odom_pred': {k[len('in.odom_pred.'):].replace('|', '/'): fx[k] for k in fx.files if k.startswith('in.odom_pred.')},
              'background': {(i, int(scenes[i][2])): fx['in.background.%d' % i] for i in n}}
    write_tables(root, scenes, tables, as_pkl=as_pkl)
    return scenes


def g13_params(cfg, root):
    data = dict(cfg['data'], data_dir=root, depth_dir=root, feats_dir=root, info_3d_dir=root, data_splits=[SPLIT])
    if cfg['odom_pred']:
        data['odom_pred_dir'] = os.path.join(root, 'odom')
    if cfg['background']:
        data['background_dir'] = os.path.join(root, 'bg')
    return {'data': data, 'use_bbox_ulbr': cfg['use_bbox_ulbr']}


def check_batch_against_g13(fx, name, batch, skip=()):
    """Every tensor the reference returned for configuration ``name`` equals the batch's, dtype included."""
    n_scenes = len(g13_scenes(fx))
    seen = 0
    for key in fx.files:
        if not key.startswith('out.%s.' % name):
            continue
        _, _, group, field, i = key.split('.')
        if (group, field) in skip:
            continue
        want, got = fx[key], batch[group][field][int(i)]
        seen += 1
        if group == 'meta':
            assert np.array_equal(np.asarray(got), want), key
            continue
        got = got.cpu()
        want = torch.from_numpy(want)
        if field == 'background':                       # stays uint8 here (the reference: int64)
            assert got.dtype == torch.uint8
            got = got.long()
        assert got.dtype == want.dtype and got.shape == want.shape, (key, got.dtype, want.dtype, got.shape, want.shape)
        assert torch.equal(got, want), key
    assert seen >= 20 * n_scenes
    for group in ('inputs', 'labels', 'meta'):          # and nothing the reference lacks, labels.feats aside
        for field in batch[group]:
            assert 'out.%s.%s.%s.0' % (name, group, field) in fx.files, (group, field)


def random_tables(n, m, seed, t=6, t_in=3):
    """Seeded tables for ``assemble_host`` / ``pf_fg_assemble``: every third instance a car, every sixth at the left border with a
    width that jumps, depths of -1, 1000000 and beyond 200, ``feat_row`` of -1."""
    g = np.random.RandomState(seed)
    x0 = g.uniform(-30, 1900, (n, 1)) + np.cumsum(g.uniform(-40, 40, (n, t)), 1)
    y0 = g.uniform(0, 900, (n, t))
    bboxes = np.stack([x0, y0, x0 + g.uniform(5, 300, (n, t)), y0 + g.uniform(5, 200, (n, t))], -1).astype(np.float32)
    k = len(bboxes[::6])                      # cars at the left border: centre and left edge inside the gap, widths that jump
    bboxes[::6, :, 0] = g.uniform(-60, -20, (k, t))
    bboxes[::6, :, 2] = bboxes[::6, :, 0] + g.uniform(5, 70, (k, t))
    depth = g.uniform(1, 260, (n, t)).astype(np.float32)
    depth[g.rand(n, t) < 0.1] = -1
    depth[g.rand(n, t) < 0.1] = 1000000
    classes = g.randint(11, 19, n).astype(np.int32)
    classes[::3] = 13
    feat_row = g.randint(0, max(m, 1), (n, t_in)).astype(np.int32)
    feat_row[g.rand(n, t_in) < 0.2] = -1
    if m == 0:
        feat_row[:] = -1
    return {'bboxes': bboxes, 'feat_mask': (g.rand(n, t) < 0.8).astype(np.uint8), 'depth': depth, 'classes': classes,
            'feat_row': feat_row, 'feat_table': g.randint(-8, 9, (m, 256, 14, 14)).astype(np.float32)}


def write_synthetic(root, n_scenes=2, seed=0, h=1024, w=2048, n_inst=None, rows=4):
    """A twin tree of ``n_scenes`` scenes with full-size backgrounds (blocky stuff / thing regions) and 3 - 5 instances each (or ``n_inst``, over
    ``rows`` feature rows per scene), in the shipped mid-term configuration; returns (scenes, params['data'] entries)."""
    g = np.random.RandomState(seed)
    scenes = [('synth', '%06d' % (i + 1), 19) for i in range(n_scenes)]
    meta = {c: [] for c in META_COLS}
    depth, cond, feats, odom, times, bgs, preds = [], [], [], [], [], {}, {}
    for i, (city, seq, frame) in enumerate(scenes):
        n = n_inst or 3 + i % 3
        cx, cy = g.uniform(200, 1800, (n, 1)) + np.cumsum(g.uniform(-8, 8, (n, 30)), 1), g.uniform(300, 800, (n, 1)) + g.uniform(-2, 2, (n, 30))
        bw, bh = g.uniform(60, 260, (n, 1)) + g.uniform(-2, 2, (n, 30)), g.uniform(60, 200, (n, 1)) + g.uniform(-2, 2, (n, 30))
        meta['bboxes'].append(np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], -1))
        mask = g.rand(n, 30) < 0.9
        mask[:, 10] = True
        meta['feat_mask'].append(mask)
        meta['feat_ind'].append(np.full((n, 30), -1, np.int64))
        meta['track_id'].append(np.arange(n) + 10 * i)
        meta['class'].append(g.randint(11, 19, n).astype(np.int64))
        depth.append(g.uniform(5, 80, (n, 30)))
        cond.append(np.where(mask, g.randint(0, rows, (n, 30)), -1).astype(np.int64))
        feats.append(g.uniform(0, 1, (rows, 256, 14, 14)).astype(np.float32))
        odom.append(g.uniform(-1, 1, (30, 5)) * [3, 0.05, 0.2, 0.02, 0.01] + [8, 0, 0.45, 0, 0])
        times.append(10.0 * i + np.cumsum(g.uniform(0.055, 0.062, 30)))
        preds['%s/%s/%d/%d' % (city, seq, frame, 10)] = (g.uniform(-1, 1, (9, 2)) * [3, 0.05] + [8, 0]).astype(np.float32)
        low = g.randint(0, 19, (h // 64, w // 64))
        low[g.rand(*low.shape) < 0.05] = 255
        bgs[(i, frame)] = low.repeat(64, 0).repeat(64, 1).astype(np.uint8)
    tables = {'meta': meta, 'depth': {'cascadedepth': depth}, 'condensed': cond, 'feats': {'%s_condensed_feats.h5' % SPLIT: feats},
              'odometry': odom, 'times': times, 'odom_pred': preds, 'background': bgs}
    write_tables(root, scenes, tables)
    data = {'data_dir': root, 'depth_dir': root, 'feats_dir': root, 'info_3d_dir': root, 'data_splits': [SPLIT],
            'odom_pred_dir': os.path.join(root, 'odom'), 'background_dir': os.path.join(root, 'bg'), 'require_most_recent': True,
            'use_cascade_depths': True, 'use_condensed_feats': True, 'use_3d_info': True, 'no_feats': False}
    return scenes, data
