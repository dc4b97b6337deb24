"""Native dataset and loader of the fg panoptic export (``export_panoptic.py``): the export path of the reference's
``FGSceneDataset`` (``data/datasets/fg_scene_dataset.py``: ``__init__`` / ``__getitem__`` / ``collate_fn`` with ``test=True`` on a
non-train split) without the reference package, ``h5py`` or - where the ``.npz`` twins exist - pandas.

``NativeFGSceneDataset`` enumerates the scenes as ``:178-211`` does and reads the reference's files under the reference's names:

    {data_dir}/{split}_seq_meta.pkl                         city, seq, frame, feat_mask, feat_ind, track_id, class, bboxes
    {depth_dir}/{split}_[cascade|mono]depth_seq_info.pkl    depth
    {feats_dir}/{split}_seq_condensed_feat_info.pkl         feat_ind                       (data.use_condensed_feats)
    {feats_dir}/{split}_condensed_feats.h5 | {split}_feats.h5 | {split}/feats.h5           '{city}/{seq}/{frame}' -> [rows,256,14,14]
    {info_3d_dir}/{split}_3d_info.pkl                       city, seq, frame, odometry, times  (data.use_3d_info)
    {odom_pred_dir}/{odom_name}_{split}.h5                  odom_io.OdometryFile
    {background_dir}/{split}/{city}/{city}_{seq}_{target:06d}_gtFine_labelIds.png

Every ``.pkl`` and ``.h5`` has an ``.npz`` twin beside it (``convert_to_npz``; the convention of ``odom_io`` / ``hop_io``): an H5's
datasets under their own names; a pickled frame's columns under theirs - one array per column, a column whose rows differ in
shape as the concatenation of its rows plus ``<column>__rows`` (the rows' lengths).  A loader takes the original when its
library imports and the file is there, else the twin, else raises an ``FGDatasetError`` that says how to convert.

Per batch the host only SELECTS (numpy: the ``has_gt`` rows and the ``bbox_inds`` columns of tables of a few rows), rebases
``feat_ind`` onto one pinned staging buffer that holds each needed feature row once, and uploads; everything ``__getitem__`` then
computes (:380-454) is one ``pf_fg_assemble`` launch for the whole batch (csrc/fg_assemble.hip).  ``batches()`` yields
``{'inputs', 'labels', 'meta'}`` in the reference's dict-of-lists layout - per-scene views split off the concatenated device
tensors, scenes with zero instances included - which ``FGModel.predict_panoptic`` takes unchanged.  ``assemble_host`` is the same
computation in torch on the CPU: the kernel's restatement inside the project, pinned to the reference by tests/golden/g13_fgscene.npz.

Two deliberate differences from the reference:
  * ``background`` stays ``uint8`` (``PanopticMerger`` takes it): the reference's int64 is eight times the upload;
  * only the T_in input steps of ``feats`` are read, and ``labels`` has no ``feats``: nothing in ``predict_*`` reads it.

Refused with an ``FGDatasetError`` naming the key: ``data.expand_test``, ``data.use_orbslam_odom``, ``data.no_feats``,
``data.input_len`` != 3, and ``test=False`` or split ``train`` (that path has the norm statistics and ``add_car_offscreen_loc``;
fg training is not built).
"""
import os

import numpy as np
import torch

from . import hop_io
from . import lib as _lib
from . import odom_io

T_IN = T_OUT = 3
T = T_IN + T_OUT
IMG_SIZE = (2048, 1024)                  # (w, h), fg_scene_dataset.py:78
PLANE = (256, 14, 14)
TARGET_INDEX = 19
BASE_INDS = np.array([4, 7, 10, 13, 16, 19])
ROWS_SUFFIX = '__rows'


class FGDatasetError(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------- files and their twins
def _twin(path):
    return os.path.splitext(path)[0] + '.npz'


def _no_file(path, lib, why):
    return FGDatasetError('%s: %s and there is no twin %s - write it once where %s is installed: '
                          'fg_dataset.convert_to_npz(%r)' % (path, why, _twin(path), lib, path))


def frame_to_arrays(frame):
    """A pickled frame's columns as npz entries (see the module docstring)."""
    out = {}
    for col in frame.columns:
        vals = list(frame[col].values)
        if vals and isinstance(vals[0], np.ndarray):
            if len({v.shape for v in vals}) == 1:
                out[col] = np.stack(vals)
            else:
                out[col] = np.concatenate(vals)
                out[col + ROWS_SUFFIX] = np.array([len(v) for v in vals], np.int64)
        else:
            out[col] = np.array(vals)
    return out


class _Table:
    """Columns of per-row values: ``t[col][i]``."""

    def __init__(self, cols):
        self.cols = cols
        self.n = len(next(iter(cols.values()))) if cols else 0

    def __getitem__(self, col):
        return self.cols[col]

    @classmethod
    def from_npz(cls, path):
        cols = {}
        with np.load(path) as z:
            for key in z.files:
                if key.endswith(ROWS_SUFFIX):
                    continue
                arr = z[key]
                if key + ROWS_SUFFIX in z.files:
                    cols[key] = np.split(arr, np.cumsum(z[key + ROWS_SUFFIX])[:-1])
                else:
                    cols[key] = list(arr)
        return cls(cols)

    @classmethod
    def from_frame(cls, frame):
        return cls({c: list(frame[c].values) for c in frame.columns})


def read_table(path):
    """``{split}_*.pkl`` (pandas) or its ``.npz`` twin."""
    if path.endswith('.npz'):
        return _Table.from_npz(path)
    why = 'no such file'
    if os.path.exists(path):
        try:
            import pandas as pd
        except ImportError:
            why = 'pandas is not installed'
        else:
            return _Table.from_frame(pd.read_pickle(path))
    if os.path.exists(_twin(path)):
        return _Table.from_npz(_twin(path))
    raise _no_file(path, 'pandas', why)


class FeatureFile:
    """``{split}_feats.h5`` / ``{split}_condensed_feats.h5`` or the ``.npz`` twin: ``rows(city, seq, frame) -> [rows,256,14,14]``."""

    def __init__(self, path):
        self.path, self._h5, self._npz = path, None, None
        why = 'no such file'
        if path.endswith('.npz'):
            self._npz = np.load(path)
            return
        if os.path.exists(path):
            try:
                import h5py
            except ImportError:
                why = 'h5py is not installed'
            else:
                self._h5 = h5py.File(path, 'r')
                return
        if not os.path.exists(_twin(path)):
            raise _no_file(path, 'h5py', why)
        self._npz = np.load(_twin(path))

    def dataset(self, city, seq, frame):
        name = '%s/%s/%d' % (city, seq, frame)                     # :443
        src = self._h5 if self._h5 is not None else self._npz
        if name not in src:
            raise FGDatasetError('%s has no feature dataset %r' % (self.path, name))
        return src[name]

    def close(self):
        for f in (self._h5, self._npz):
            if f is not None:
                f.close()


def convert_to_npz(path, npz_path=None):
    """The ``.npz`` twin of one of the dataset's files: a pickled frame (needs pandas) or an H5 file (needs h5py)."""
    npz_path = npz_path or _twin(path)
    if path.endswith('.pkl'):
        import pandas as pd
        np.savez_compressed(npz_path, **frame_to_arrays(pd.read_pickle(path)))
        return npz_path
    return odom_io.convert_h5_to_npz(path, npz_path)


# ---------------------------------------------------------------------------------------------- the computation, on the host
def assemble_host(bboxes, feat_mask, depth, classes, feat_row, feat_table, use_ulbr=False, max_depth=None, filter_car_gap=None,
                  img_w=IMG_SIZE[0]):
    """What ``pf_fg_assemble`` computes, in torch on the CPU, in the reference's operations and order
    (fg_scene_dataset.py:380-454, ``_filter_car_gap`` :300-340 vectorised over the instances; ``.float()`` first).
    Arguments and results as ``device_assemble``."""
    b = torch.as_tensor(bboxes).float().clone()
    n, t_all = b.shape[:2]
    if not use_ulbr:                                                                # data_utils.convert_bbox_ulbr_cwh
        b = torch.stack([(b[..., 0] + b[..., 2]) / 2, (b[..., 1] + b[..., 3]) / 2, b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]], -1)
    bm = torch.as_tensor(feat_mask).bool().clone()
    fm = bm.clone()
    cls = torch.as_tensor(classes).long()
    if filter_car_gap is not None:
        gap = filter_car_gap
        car = cls == 13
        found0, found1, zero_rest, have_past = (torch.zeros(n, dtype=torch.bool) for _ in range(4))
        past = torch.zeros(n)
        for t in range(t_all):
            act = car & ~zero_rest & bm[:, t]
            x0, x1 = b[:, t, 0], b[:, t, 2]                                         # cx and w unless use_ulbr (kept as is)
            found0 = found0 | (act & (x0 < gap))
            found1 = found1 | (act & (x1 > img_w - gap))
            for on, cur, far in ((act & found0, x1, lambda: x1 > past + gap), (act & found1, x0, lambda: x0 < past - gap)):
                zero_rest = zero_rest | (on & have_past & far())
                past = torch.where(on, cur, past)
                have_past = have_past | on
            z = car & zero_rest
            bm[z, t] = False
            fm[z, t] = False
            b[z, t] = 0
    vel = torch.cat([torch.zeros(n, 1, 4), b[:, 1:] - b[:, :-1]], dim=1)
    vel[:, 1:] *= (bm[:, :-1] * bm[:, 1:]).unsqueeze(-1)
    vel_mask = torch.cat([torch.zeros(n, 1, dtype=torch.bool), bm[:, 1:] * bm[:, :-1]], dim=1)
    d = torch.as_tensor(depth).float().unsqueeze(-1)
    dm = (d != -1) & (d != 1000000)
    if max_depth is not None:
        dm = dm * (d <= max_depth)
    dvel = torch.cat([torch.zeros(n, 1, 1), d[:, 1:] - d[:, :-1]], dim=1)
    dvel[:, 1:] *= (dm[:, :-1] * dm[:, 1:])
    inp_cls = cls - 11
    rows = torch.as_tensor(feat_row).long()
    table = torch.as_tensor(feat_table).float()
    feats = torch.zeros((n, rows.shape[1]) + PLANE)
    valid = (rows >= 0) & (rows < table.shape[0])
    feats[valid] = table[rows[valid]]
    return {'trajectories': torch.cat([b, vel], -1), 'bbox_masks': bm, 'bbox_vel_masks': vel_mask, 'feat_masks': fm,
            'depths': torch.cat([d, dvel], -1), 'depth_masks': dm.squeeze(-1), 'classes': inp_cls,
            'one_hot_classes': (inp_cls[:, None] == torch.arange(8)[None, :]).float(), 'final_bboxes': b[:, -1].clone(),
            'feats': feats}


def device_assemble(bboxes, feat_mask, depth, classes, feat_row, feat_table, use_ulbr=False, max_depth=None, filter_car_gap=None,
                    img_w=IMG_SIZE[0]):
    """One ``pf_fg_assemble`` launch on the current stream.  ``bboxes [N,T,4]`` f32 ulbr, ``feat_mask [N,T]`` u8 / bool,
    ``depth [N,T]`` f32, ``classes [N]`` i32 trainIds, ``feat_row [N,T_in]`` i32, ``feat_table [M,256,14,14]`` f32 - on the device.
    Returns ``trajectories [N,T,8]``, ``bbox_masks`` / ``bbox_vel_masks`` / ``feat_masks`` / ``depth_masks [N,T]`` bool,
    ``depths [N,T,2]``, ``classes [N]`` i64 (class - 11), ``one_hot_classes [N,8]``, ``final_bboxes [N,4]``,
    ``feats [N,T_in,256,14,14]``."""
    L = _lib.load()
    want = (('bboxes', bboxes, torch.float32, 3), ('feat_mask', feat_mask, None, 2), ('depth', depth, torch.float32, 2),
            ('classes', classes, torch.int32, 1), ('feat_row', feat_row, torch.int32, 2), ('feat_table', feat_table, torch.float32, 4))
    for name, t, dt, dim in want:
        _lib.require_cuda(t, name)
        if (dt is not None and t.dtype != dt) or t.dim() != dim:
            raise _lib.PfError('%s must be %d-d %s (got %s %s)' % (name, dim, dt, tuple(t.shape), t.dtype))
    if feat_mask.dtype not in (torch.uint8, torch.bool):
        raise _lib.PfError('feat_mask must be uint8 or bool (got %s)' % feat_mask.dtype)
    n, t_all = bboxes.shape[:2]
    t_in, m = feat_row.shape[1], feat_table.shape[0]
    if tuple(bboxes.shape) != (n, t_all, 4) or tuple(feat_mask.shape) != (n, t_all) or tuple(depth.shape) != (n, t_all) or \
            tuple(classes.shape) != (n,) or feat_row.shape[0] != n or tuple(feat_table.shape[1:]) != PLANE:
        raise _lib.PfError('pf_fg_assemble: shapes disagree (bboxes %s, feat_mask %s, depth %s, classes %s, feat_row %s, feat_table %s)'
                           % tuple(tuple(x.shape) for _, x, _, _ in want))
    dev = bboxes.device
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)      # noqa: E731
    out = {'trajectories': new((n, t_all, 8), torch.float32), 'bbox_masks': new((n, t_all), torch.uint8),
           'bbox_vel_masks': new((n, t_all), torch.uint8), 'feat_masks': new((n, t_all), torch.uint8),
           'depths': new((n, t_all, 2), torch.float32), 'depth_masks': new((n, t_all), torch.uint8),
           'classes': new((n,), torch.int64), 'one_hot_classes': new((n, 8), torch.float32),
           'final_bboxes': new((n, 4), torch.float32), 'feats': new((n, t_in) + PLANE, torch.float32)}
    ptr = lambda x: x.data_ptr() if x.numel() else None                   # noqa: E731
    rc = L.pf_fg_assemble(ptr(bboxes), ptr(feat_mask), ptr(depth), ptr(classes), ptr(feat_row), ptr(feat_table), n, t_all, t_in, m,
                          int(bool(use_ulbr)), -1.0 if max_depth is None else float(max_depth),
                          -1.0 if filter_car_gap is None else float(filter_car_gap), int(img_w),
                          *[ptr(out[k]) for k in ('trajectories', 'bbox_masks', 'bbox_vel_masks', 'feat_masks', 'depths',
                                                  'depth_masks', 'classes', 'one_hot_classes', 'final_bboxes', 'feats')],
                          _lib.stream_ptr())
    _lib.check(rc, 'pf_fg_assemble')
    for k in ('bbox_masks', 'bbox_vel_masks', 'feat_masks', 'depth_masks'):
        out[k] = out[k].view(torch.bool)
    return out


# ---------------------------------------------------------------------------------------------- the dataset
class NativeFGSceneDataset:
    """One entry per row of ``{split}_seq_meta``.  ``scene(i)`` is the host's selection for one scene, ``stage(indices)`` the
    tables of a batch, ``batches()`` the loader; ``len()`` as the reference's."""

    def __init__(self, split, params, test=False):
        data = params['data']
        for key in ('expand_test', 'use_orbslam_odom', 'no_feats'):
            if data.get(key):
                raise FGDatasetError('data.%s is not supported by the native fg dataset' % key)
        if data.get('input_len', 3) != 3:
            raise FGDatasetError('data.input_len = %r is not supported (3, as in the reference)' % data.get('input_len'))
        if not test:
            raise FGDatasetError('test=False is not supported: the native fg dataset restates the export path only (fg training '
                                 'is not built)')
        if split == 'train':
            raise FGDatasetError('split \'train\' is not supported: it carries the norm statistics and add_car_offscreen_loc of '
                                 'fg training, which is not built')
        self.split, self.test = split, test
        self.data_dir = data['data_dir']
        self.depth_dir = data['depth_dir']
        self.use_3d_info = data.get('use_3d_info')
        self.info_3d_dir = data.get('info_3d_dir', self.data_dir)
        self.odom_pred_dir = data.get('odom_pred_dir')
        if self.odom_pred_dir is not None:
            self.odom_pred_dir = os.path.join(self.odom_pred_dir, '%s_%s.h5' % (data.get('odom_name', 'predicted_odometry'), split))
        self.filter_car_gap = data.get('filter_car_gap')
        self.max_depth = data.get('max_depth')
        self.background_dir = data.get('background_dir')
        if self.background_dir is not None:
            self.background_dir = os.path.join(self.background_dir, split)
        self.require_most_recent = data.get('require_most_recent')
        self.output_ind = data.get('output_ind')
        if self.output_ind is not None and self.output_ind not in (0, 1, 2):
            raise FGDatasetError('data.output_ind = %r is not supported (None, or 0 .. 2)' % (self.output_ind,))
        self.use_ulbr = params.get('use_bbox_ulbr')
        self.img_size = list(IMG_SIZE)
        data['num_classes'] = 19
        data['odom_size'] = 5
        data['img_size'] = torch.FloatTensor(self.img_size)
        self.meta = read_table(os.path.join(self.data_dir, '%s_seq_meta.pkl' % split))
        kind = 'cascadedepth' if data.get('use_cascade_depths') else 'monodepth' if data.get('use_monodepth') else 'depth'
        self.depth_data = read_table(os.path.join(self.depth_dir, '%s_%s_seq_info.pkl' % (split, kind)))
        feats_dir = data.get('feats_dir')
        self.use_condensed_feats = data.get('use_condensed_feats')
        self.feats_meta = None
        if self.use_condensed_feats:
            feats_path = os.path.join(feats_dir, '%s_condensed_feats.h5' % split)
            self.feats_meta = read_table(os.path.join(feats_dir, '%s_seq_condensed_feat_info.pkl' % split))
        else:
            feats_path = os.path.join(feats_dir, '%s_feats.h5' % split)
            if not os.path.exists(feats_path) and not os.path.exists(_twin(feats_path)):
                feats_path = os.path.join(feats_dir, split, 'feats.h5')
        self.feats = FeatureFile(feats_path)
        self.data3d = self.row3d = None
        if self.use_3d_info:
            self.data3d = read_table(os.path.join(self.info_3d_dir, '%s_3d_info.pkl' % split))
            self.row3d = {(str(c), str(s), int(f)): i for i, (c, s, f) in
                          reversed(list(enumerate(zip(self.data3d['city'], self.data3d['seq'], self.data3d['frame']))))}
        self.odom_file = None
        if self.odom_pred_dir is not None and self.use_3d_info:
            path = self.odom_pred_dir
            if not os.path.exists(path) and os.path.exists(_twin(path)):
                path = _twin(path)
            self.odom_file = odom_io.OdometryFile(path)
        # :207-211: one entry per scene (the reference's start_fr field is never read and is not kept)
        inds = BASE_INDS + 6 if self.output_ind == 0 else BASE_INDS
        self.instance_inds = [(i, inds) for i in range(self.meta.n)]
        self._feat_stage = self._bg_stage = self._staged = None
        print('TOTAL NUM INSTANCES: ', len(self.instance_inds))

    def __len__(self):
        return len(self.instance_inds)

    # ---- host selection ---------------------------------------------------------------------------
    def scene(self, idx):
        """:343-379 and the file reads of :440-510 for one scene, numpy only: the selected tables, the feature rows it needs, its
        odometry and the path of its background."""
        row, fr = self.instance_inds[idx]
        city, seq, frame = str(self.meta['city'][row]), str(self.meta['seq'][row]), int(self.meta['frame'][row])
        mask_all = np.asarray(self.meta['feat_mask'][row]).astype(bool)
        fm = mask_all[:, fr]
        src = self.feats_meta if self.use_condensed_feats else self.meta
        feat_ind = np.asarray(src['feat_ind'][row])[:, fr]
        has_gt = fm[:, T_IN - 1] if self.require_most_recent else fm[:, :T_IN].sum(1) > 0
        feat_ind = feat_ind[has_gt][:, :T_IN].astype(np.int64)
        n = int(has_gt.sum())
        out_ind = self.output_ind if self.output_ind is not None else -1
        s = {'city': city, 'seq': seq, 'frame': frame, 'fr_inds': fr, 'n': n,
             'target_frame': int(frame - TARGET_INDEX + fr[T_IN:][out_ind]),
             'track_id': np.asarray(self.meta['track_id'][row])[has_gt],
             'feat_mask': fm[has_gt].astype(np.uint8),
             'bboxes': np.asarray(self.meta['bboxes'][row])[has_gt][:, fr].astype(np.float32).reshape(n, T, 4),
             'depth': np.asarray(self.depth_data['depth'][row])[has_gt][:, fr].astype(np.float32).reshape(n, T),
             'classes': np.asarray(self.meta['class'][row])[has_gt].astype(np.int32).reshape(n),
             'feat_ind': feat_ind, 'feat_rows': None}
        if n:
            dset = self.feats.dataset(city, seq, frame)
            rows = dset.shape[0]
            bad = (feat_ind < -1) | (feat_ind >= rows)
            if bad.any():
                raise FGDatasetError('%s/%s/%d: feat_ind %d lies outside [-1, %d), the rows of the scene\'s feature dataset'
                                     % (city, seq, frame, int(feat_ind[bad][0]), rows))
            need = np.unique(feat_ind[feat_ind >= 0])
            s['feat_rows'] = (need, np.asarray(dset[list(need)] if len(need) else np.zeros((0,) + PLANE), dtype=np.float32))
        if self.use_3d_info:
            key = (city, seq, frame)
            if key not in self.row3d:
                raise FGDatasetError('no 3d info for %s/%s/%d' % key)
            r3 = self.row3d[key]
            odometry = np.asarray(self.data3d['odometry'][r3])
            if self.odom_file is not None:                                          # :465-493
                times = np.asarray(self.data3d['times'][r3])[fr[0]:fr[T_IN - 1] + 1]
                s['odometry'] = odom_io.fg_odometry(odometry[fr[:T_IN]], self.odom_file.rows(city, seq, frame, fr[T_IN - 1]), times)
            else:
                s['odometry'] = odometry[fr].astype(np.float32)
        if self.background_dir is not None:
            s['background_path'] = os.path.join(self.background_dir, city, hop_io.LABEL_PNG % (city, seq, s['target_frame']))
        return s

    def stage(self, indices, feat_out=None):
        """The tables of one batch on the host: the scenes' selections concatenated, ``feat_row`` = ``feat_ind`` rebased onto
        ``feat_table``, which holds each needed feature row once (written into ``feat_out(M)`` when given)."""
        scenes = [self.scene(i) for i in indices]
        counts = [s['n'] for s in scenes]
        cat = lambda k, shape, dt: np.concatenate([s[k] for s in scenes]) if scenes else np.zeros(shape, dt)      # noqa: E731
        m = sum(len(s['feat_rows'][0]) for s in scenes if s['feat_rows'] is not None)
        table = feat_out(m) if feat_out is not None else np.zeros((m,) + PLANE, np.float32)
        feat_row, base = [], 0
        for s in scenes:
            fi = s['feat_ind']
            if s['feat_rows'] is not None:
                need, planes = s['feat_rows']
                table[base:base + len(need)] = planes
                fi = np.where(fi >= 0, base + np.searchsorted(need, fi), -1)
                base += len(need)
            feat_row.append(fi.astype(np.int32).reshape(-1, T_IN))
        return {'scenes': scenes, 'counts': counts, 'bboxes': cat('bboxes', (0, T, 4), np.float32),
                'feat_mask': cat('feat_mask', (0, T), np.uint8), 'depth': cat('depth', (0, T), np.float32),
                'classes': cat('classes', (0,), np.int32), 'feat_row': np.concatenate(feat_row) if feat_row else np.zeros((0, T_IN), np.int32),
                'feat_table': table[:m]}

    def assemble_kwargs(self):
        return {'use_ulbr': bool(self.use_ulbr), 'max_depth': self.max_depth, 'filter_car_gap': self.filter_car_gap,
                'img_w': self.img_size[0]}

    def make_batch(self, staged, asm, odometry, backgrounds):
        """The reference's ``collate_fn`` layout from the assembled ``[N, ...]`` tensors: per-scene views, nothing copied."""
        counts, scenes = staged['counts'], staged['scenes']
        dev = asm['trajectories'].device
        n = sum(counts)
        split = lambda t: list(t.split(counts))                                     # noqa: E731
        out_ind = self.output_ind if self.output_ind is not None else T_OUT - 1
        inds = torch.full((n,), out_ind, dtype=torch.int64, device=dev)
        img = torch.tensor(self.img_size, dtype=torch.float32, device=dev).repeat(n, 1)
        dm = asm['depth_masks'].unsqueeze(-1)
        inputs = {'feat_masks': split(asm['feat_masks']), 'bbox_masks': split(asm['bbox_masks']),
                  'bbox_vel_masks': split(asm['bbox_vel_masks']), 'trajectories': split(asm['trajectories'][:, :T_IN]),
                  'depths': split(asm['depths'][:, :T_IN]), 'depth_masks': split(dm[:, :T_IN]), 'classes': split(asm['classes']),
                  'one_hot_classes': split(asm['one_hot_classes']), 'final_bboxes': split(asm['final_bboxes']),
                  'img_size': split(img), 'feats': split(asm['feats'])}
        labels = {'output_inds': split(inds), 'bbox_output_inds': split(inds.clone()), 'trajectories': split(asm['trajectories'][:, T_IN:]),
                  'depths': split(asm['depths'][:, T_IN:]), 'depth_masks': split(dm[:, T_IN:])}
        if odometry is not None:
            inputs['odometry'] = [odometry[b].unsqueeze(0).expand(c, -1, -1) for b, c in enumerate(counts)]
        if backgrounds is not None:
            inputs['background'] = list(backgrounds)
        meta = {k: [s[k] for s in scenes] for k in ('city', 'seq', 'frame', 'track_id', 'fr_inds', 'target_frame')}
        return {'inputs': inputs, 'labels': labels, 'meta': meta}

    def read_backgrounds(self, scenes):
        """[B,H,W] u8 of the scenes' background maps (None without ``data.background_dir``)."""
        if self.background_dir is None or not scenes:
            return None
        maps = []
        for s in scenes:
            arr = hop_io.read_png(s['background_path'])
            if arr.ndim != 2 or arr.dtype != np.uint8:
                raise FGDatasetError('%s: expected an 8-bit single-channel label map, got %s %s' % (s['background_path'], arr.shape, arr.dtype))
            maps.append(arr)
        return np.stack(maps)

    def host_batch(self, indices):
        """A batch assembled by ``assemble_host`` on the CPU, in the layout ``batches()`` yields."""
        st = self.stage(indices)
        tens = {k: torch.from_numpy(np.ascontiguousarray(st[k])) for k in ('bboxes', 'feat_mask', 'depth', 'classes', 'feat_row', 'feat_table')}
        asm = assemble_host(**tens, **self.assemble_kwargs())
        odom = torch.from_numpy(np.stack([s['odometry'] for s in st['scenes']])) if self.use_3d_info and st['scenes'] else None
        bg = self.read_backgrounds(st['scenes'])
        return self.make_batch(st, asm, odom, torch.from_numpy(bg) if bg is not None else None)

    # ---- device loader ----------------------------------------------------------------------------
    def _pinned(self, name, shape, dtype):
        """A pinned staging buffer of at least ``shape``, reused between batches (grown when a batch needs more rows)."""
        cur = getattr(self, name)
        if cur is None or cur.shape[0] < shape[0] or tuple(cur.shape[1:]) != tuple(shape[1:]):
            cur = torch.empty((max(shape[0], 1),) + tuple(shape[1:]), dtype=dtype).pin_memory()
            setattr(self, name, cur)
        return cur

    def stage_pinned(self, indices):
        """Stage 1 (host): the batch's tables, its feature rows and its backgrounds, the last two in pinned staging buffers."""
        if self._staged is not None:
            self._staged.synchronize()          # the previous batch's uploads have read the pinned buffers
        st = self.stage(indices, feat_out=lambda m: self._pinned('_feat_stage', (m,) + PLANE, torch.float32).numpy())
        bg = self.read_backgrounds(st['scenes'])
        st['has_background'] = bg is not None
        if bg is not None:
            self._pinned('_bg_stage', bg.shape, torch.uint8).numpy()[:len(bg)] = bg
        return st

    def upload(self, st, device='cuda'):
        """Stage 2: the staged batch to ``device`` (the two pinned buffers asynchronously; the tables are a few hundred bytes)."""
        scenes, m = st['scenes'], st['feat_table'].shape[0]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)         # noqa: E731
        dev = {k: up(st[k]) for k in ('bboxes', 'feat_mask', 'depth', 'classes', 'feat_row')}
        dev['feat_table'] = self._feat_stage[:m].to(device, non_blocking=True) if m else torch.empty((0,) + PLANE, device=device)
        odom = up(np.stack([s['odometry'] for s in scenes])) if self.use_3d_info and scenes else None
        bg = self._bg_stage[:len(scenes)].to(device, non_blocking=True) if st['has_background'] else None
        self._staged = torch.cuda.Event()
        self._staged.record()
        return dev, odom, bg

    def device_batch(self, indices, device='cuda'):
        """Stage (host), upload, one ``pf_fg_assemble`` launch -> the batch on ``device``."""
        st = self.stage_pinned(indices)
        dev, odom, bg = self.upload(st, device)
        return self.make_batch(st, device_assemble(**dev, **self.assemble_kwargs()), odom, bg)

    def batches(self, batch_size, device='cuda'):
        """Sequential batches of ``batch_size`` scenes, as the reference's DataLoader orders an export."""
        for i in range(0, len(self), batch_size):
            yield self.device_batch(range(i, min(i + batch_size, len(self))), device)

    def close(self):
        self.feats.close()
        if self.odom_file is not None:
            self.odom_file.close()


def build_dataset(params, test=False):
    """``data.build_dataset`` of the reference for ``task: fg``: {split: dataset}."""
    return {split: NativeFGSceneDataset(split, params, test=test) for split in params['data']['data_splits']}
