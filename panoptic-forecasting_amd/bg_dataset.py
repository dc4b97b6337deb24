"""Native dataset and loader for ``task: bg`` training (``train_bg.py --dataset native``): the reference's ``BGDataset``
(``data/datasets/bg_dataset.py``) without the reference package, ``cv2``, ``torchvision`` or ``cityscapesscripts``.

``NativeBGDataset`` enumerates the samples as ``bg_dataset.py:78-111`` does (sorted, where the reference takes ``os.listdir``
/ ``glob`` order) and decodes PNGs; nothing else runs on the host.  ``NativeBatches`` puts it behind the ``batches(epoch)``
interface of ``train_bg.py``:

    thread pool: PNG -> pinned staging      side stream: staging -> device       current stream: pf_bg_augment
    (one task per file, batch k + 1)         (batch k + 1, after batch k's        (after an event wait) -> the u8 / f32 batch
                                              sources were consumed)               pf_train_forward_backward takes as is

The joint random scale / pad / crop / resize / flip and the depth decode are ONE kernel launch per batch (bg_augment.py,
csrc/bg_augment.hip); batch k + 1 is decoded and uploaded while batch k trains.  A sample's random parameters come from
``random.Random(f(seed, epoch, dataset index))``, so a batch holds the same bits whatever the number of threads, and a
sample is transformed the same way whichever rank draws it.
"""
import glob
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import bg_augment
from . import hop_io

MAX_THREADS = 16        # a training job gets 16 CPUs; never sized from the machine's CPU count
NORM_KEY = 'data.depth_norm_params_file'


class BGDatasetError(RuntimeError):
    pass


def _read_u8(path):
    arr = hop_io.read_png(path)
    if arr.ndim != 2 or arr.dtype != np.uint8:
        raise BGDatasetError('%s: expected an 8-bit single-channel label map, got %s %s' % (path, arr.shape, arr.dtype))
    return arr


def _read_u16(path):
    arr = hop_io.read_png(path)
    if arr.ndim != 2:
        raise BGDatasetError('%s: expected a single-channel 16-bit depth map, got shape %s' % (path, arr.shape))
    return arr.astype(np.uint16, copy=False)


def resolve_depth_norm_params(data):
    """``[mean, std]`` as floats from ``data.depth_norm_params_file`` (``torch.load``, what the reference saved at
    ``bg_dataset.py:135``) or from ``data.depth_norm_params`` of the config.  The reference computes them from the depth
    H5 when the file is missing (:115-139); this loader refuses."""
    path = data.get('depth_norm_params_file')
    if path and os.path.exists(path):
        mean, std = torch.load(path, map_location='cpu')
        return [float(mean), float(std)]
    dn = data.get('depth_norm_params')
    if dn is not None:
        return [float(dn[0]), float(dn[1])]
    raise BGDatasetError('%s = %r does not exist and the config holds no data.depth_norm_params: computing the depth '
                         'normalisation from the depth file is not supported here - point %s at the file the reference '
                         'saved, or set data.depth_norm_params: [mean, std]' % (NORM_KEY, path, NORM_KEY))


class NativeBGDataset:
    """``samples``: one dict per (ground-truth frame, ``data_dir`` group / ``gap_len``) with ``gt_file``, ``data_files`` (T label
    PNGs), ``depth_files`` (T u16 PNGs, or None), ``city``, ``seq``, ``frame``, ``start_fr``, ``target_frame``."""

    def __init__(self, split, params, test=False):
        data = params['data']
        self.split, self.test = split, test
        self.train = split == 'train' and not test
        if data.get('resize_h') is not None or data.get('resize_w') is not None:
            raise BGDatasetError('data.resize_w / data.resize_h (the pre-resize) are not supported by --dataset native')
        self.inp_size = int(data.get('data_inp_size', 3))
        data_dir = data['data_dir']
        dirs = [os.path.join(d, split) for d in (data_dir if isinstance(data_dir, list) else [data_dir])]
        self.groups = [dirs[st:st + self.inp_size] for st in range(0, len(dirs), self.inp_size)]
        self.gap_len = list(data.get('gap_len', [9]))
        self.gt_dir = os.path.join(data['gt_dir'], split)
        self.use_depths = bool(data.get('use_depths'))
        self.min_depth, self.max_depth = float(data.get('min_depth') or 0.), float(data.get('max_depth') or 0.)
        self.num_classes = data['num_classes'] = 11 if data.get('only_background') else 19
        self.no_resize_crop = bool(data.get('no_resize_crop'))
        self.crop_size = data.get('crop_size')
        self.scale_min, self.scale_max = data.get('scale_min'), data.get('scale_max')
        if self.train and not self.no_resize_crop and None in (self.crop_size, self.scale_min, self.scale_max):
            raise BGDatasetError('training needs data.crop_size, data.scale_min and data.scale_max (or data.no_resize_crop)')
        self.h5 = None
        if self.use_depths:
            try:
                import h5py  # noqa: F401
                self.h5_path = data['depth_h5_path'] % split
            except ImportError:
                self.h5_path = None         # per-frame u16 PNGs next to the labels (export_bg.py --save_depth_as_png)
            if self.train and not params.get('continue_training'):
                data['depth_norm_params'] = resolve_depth_norm_params(data)
        self.samples = []
        for city_dir in sorted(os.listdir(self.gt_dir)):
            for gt_file in sorted(glob.glob(os.path.join(self.gt_dir, city_dir, '*_labelTrainIds.png'))):
                parts = os.path.basename(gt_file).split('_')
                city, seq, frame = parts[0], parts[1], int(parts[2])
                for group, gap in zip(self.groups, self.gap_len):
                    files = [os.path.join(d, city, hop_io.LABEL_PNG % (city, seq, frame)) for d in group]
                    for f in files:
                        if not os.path.exists(f):
                            raise IOError('Could not find data file: %s' % f)
                    depth_files = None
                    if self.use_depths and self.h5_path is None:
                        depth_files = [os.path.join(d, city, hop_io.DEPTH_PNG % (city, seq, frame)) for d in group]
                    self.samples.append({'gt_file': gt_file, 'data_files': files, 'depth_files': depth_files, 'city': city,
                                         'seq': seq, 'frame': frame, 'start_fr': (9 - gap) / 3, 'target_frame': frame})
        self.T = len(self.groups[0]) if self.groups else 0
        self._shape = None

    def __len__(self):
        return len(self.samples)

    def source_shape(self):
        """(H, W) of the files, read from the first ground-truth map; every file of the dataset must have it."""
        if self._shape is None:
            self._shape = tuple(_read_u8(self.samples[0]['gt_file']).shape)
        return self._shape

    def decode_tasks(self, idx, seg, label, depth):
        """The decode of sample ``idx`` as independent callables, one per file, each writing its plane of the given host
        arrays ``seg [T,H,W]`` u8, ``label [H,W]`` u8, ``depth [T,H,W]`` u16 (None without depths)."""
        s = self.samples[idx]

        def put(dst, read, path):
            arr = read(path)
            if arr.shape != dst.shape:
                raise BGDatasetError('%s is %s, the dataset is %s' % (path, arr.shape, dst.shape))
            dst[...] = arr

        tasks = [lambda: put(label, _read_u8, s['gt_file'])]
        tasks += [lambda t=t, f=f: put(seg[t], _read_u8, f) for t, f in enumerate(s['data_files'])]
        if depth is not None:
            if s['depth_files'] is not None:
                tasks += [lambda t=t, f=f: put(depth[t], _read_u16, f) for t, f in enumerate(s['depth_files'])]
            else:       # one [H,W,T] stack per sample (bg_dataset.py:183-187)
                def read_stack(_path):
                    return np.moveaxis(self._h5().read(s['city'], s['seq'], s['frame'], s['start_fr']), 2, 0)
                tasks.append(lambda: put(depth, read_stack, self.h5_path))
        return tasks

    def _h5(self):
        if self.h5 is None:
            self.h5 = hop_io.DepthH5(self.h5_path)
        return self.h5

    def draw(self, seed, epoch, idx):
        """The random parameters of sample ``idx`` in ``epoch``: a function of (seed, epoch, idx) alone."""
        if not self.train:
            return None
        rng = random.Random((int(seed) * 1000003 + int(epoch)) * 1000003 + int(idx))
        h, w = self.source_shape()
        if self.no_resize_crop:
            return bg_augment.draw_flip(rng)
        return bg_augment.draw_params(rng, w, h, self.crop_size, self.scale_min, self.scale_max)

    def out_shape(self):
        h, w = self.source_shape()
        if not self.train or self.no_resize_crop:
            return h, w
        ow, oh = bg_augment._pair(self.crop_size)
        return oh, ow


def build_dataset(params, test=False):
    """``data.build_dataset`` of the reference for ``task: bg``: {split: dataset}; injects ``data.num_classes`` and
    ``data.depth_norm_params`` (bg_dataset.py:62-66,140-141)."""
    return {split: NativeBGDataset(split, params, test=test) for split in params['data']['data_splits']}


class _Slot:
    """One batch in flight: pinned staging, device sources, device tables."""

    def __init__(self, bs, t, h, w, oh, ow, depths):
        pin = lambda shape, dt: torch.empty(shape, dtype=dt).pin_memory()      # noqa: E731
        dev = lambda x: torch.empty_like(x, device='cuda')                     # noqa: E731
        self.h_seg, self.h_lab = pin((bs, t, h, w), torch.uint8), pin((bs, h, w), torch.uint8)
        self.h_dep = pin((bs, t, h, w), torch.int16) if depths else None        # u16 bit patterns
        self.h_tab = pin((bs, 2 * oh + 2 * ow), torch.int32)
        self.d_seg, self.d_lab, self.d_tab = dev(self.h_seg), dev(self.h_lab), dev(self.h_tab)
        self.d_dep = dev(self.h_dep) if depths else None
        self.uploaded, self.consumed = torch.cuda.Event(), None
        self.indices = []


class NativeBatches:
    """``batches(epoch)`` over a ``NativeBGDataset``.  Training: one ``randperm`` per pass, ``drop_last``, cycled to
    ``steps_per_epoch * accumulate_steps`` when that key is set (``train.py:104-116``); validation: sequential.  Under
    ``torchrun`` rank r takes every ``world``-th entry of the order, starting at r."""

    def __init__(self, dataset, params, rank, world, train, threads=None):
        tr = params.get('training', {})
        self.ds, self.rank, self.world, self.train = dataset, rank, world, train
        self.seed = int(params.get('seed', 1))
        self.bs = int(tr.get('batch_size', 1000)) if train else int(tr.get('val_batch_size') or tr.get('batch_size', 1000))
        if threads is None:
            threads = tr.get('num_data_workers', 0) if train else tr.get('num_val_data_workers', tr.get('num_data_workers', 0))
        self.threads = max(1, min(int(threads or 0), MAX_THREADS))
        steps = tr.get('steps_per_epoch') if train else None
        self.steps = int(steps) * max(1, int(tr.get('accumulate_steps', 1))) if steps else None
        self.per_rank = len(dataset) // world if train else len(range(rank, len(dataset), world))
        if not train:
            self.bs = max(1, min(self.bs, self.per_rank))      # staging is sized by the batch: not by the default of 1000
        self._slots = None
        self._pool = None
        self._stream = None

    def __len__(self):
        if self.steps:
            return self.steps
        return self.per_rank // self.bs if self.train else (self.per_rank + self.bs - 1) // self.bs

    # ---- order ------------------------------------------------------------------------------------
    def _pass_batches(self, epoch, pas):
        n = len(self.ds)
        if self.train:
            g = torch.Generator().manual_seed((self.seed * 1000003 + int(epoch)) * 1009 + pas)
            order = torch.randperm(n, generator=g).tolist()[:self.per_rank * self.world]
            mine = order[self.rank::self.world]
            return [mine[i:i + self.bs] for i in range(0, len(mine) - self.bs + 1, self.bs)]
        mine = list(range(self.rank, n, self.world))
        return [mine[i:i + self.bs] for i in range(0, len(mine), self.bs)]

    def index_batches(self, epoch):
        """The lists of dataset indices of this rank's batches in ``epoch``, in order."""
        first = self._pass_batches(epoch, 0)
        if self.steps is None:
            return first
        if not first:
            raise BGDatasetError('the dataset holds fewer samples per rank (%d) than one batch (%d)' % (self.per_rank, self.bs))
        out, pas = list(first), 0
        while len(out) < self.steps:
            pas += 1
            out += self._pass_batches(epoch, pas)
        return out[:self.steps]

    # ---- stages -----------------------------------------------------------------------------------
    def _setup(self):
        if self._slots is None:
            h, w = self.ds.source_shape()
            oh, ow = self.ds.out_shape()
            self._slots = [_Slot(self.bs, self.ds.T, h, w, oh, ow, self.ds.use_depths) for _ in range(2)]
            self._pool = ThreadPoolExecutor(self.threads)
            self._stream = torch.cuda.Stream()

    def decode(self, slot, indices, epoch):
        """Stage 1 (host): the files of ``indices`` into ``slot``'s pinned staging, one pool task per file, and the tables."""
        seg, lab = slot.h_seg.numpy(), slot.h_lab.numpy()
        dep = slot.h_dep.numpy().view(np.uint16) if slot.h_dep is not None else None
        tasks = []
        for b, idx in enumerate(indices):
            tasks += self.ds.decode_tasks(idx, seg[b], lab[b], dep[b] if dep is not None else None)
        futures = [self._pool.submit(t) for t in tasks]
        h, w = self.ds.source_shape()
        tab = slot.h_tab.numpy()
        for b, idx in enumerate(indices):
            tab[b] = np.concatenate(bg_augment.build_tables(self.ds.draw(self.seed, epoch, idx), w, h, self.ds.crop_size))
        for f in futures:
            f.result()
        slot.indices = list(indices)

    def upload(self, slot):
        """Stage 2 (side stream): staging -> device, once the kernel that read the slot's previous contents has run."""
        n = len(slot.indices)
        with torch.cuda.stream(self._stream):
            if slot.consumed is not None:
                self._stream.wait_event(slot.consumed)
            slot.d_seg[:n].copy_(slot.h_seg[:n], non_blocking=True)
            slot.d_lab[:n].copy_(slot.h_lab[:n], non_blocking=True)
            slot.d_tab[:n].copy_(slot.h_tab[:n], non_blocking=True)
            if slot.d_dep is not None:
                slot.d_dep[:n].copy_(slot.h_dep[:n], non_blocking=True)
            slot.uploaded.record(self._stream)

    def augment(self, slot):
        """Stage 3 (current stream): ``pf_bg_augment`` after the upload's event -> the batch dict."""
        n = len(slot.indices)
        oh, ow = self.ds.out_shape()
        cur = torch.cuda.current_stream()
        cur.wait_event(slot.uploaded)
        tab = slot.d_tab[:n]
        y_map, x_map = tab[:, :oh].contiguous(), tab[:, oh:oh + ow].contiguous()
        y_arr, x_arr = tab[:, oh + ow:2 * oh + ow].contiguous(), tab[:, 2 * oh + ow:].contiguous()
        seg, lab, dep, msk = bg_augment.device_augment(slot.d_seg[:n], slot.d_lab[:n], slot.d_dep[:n] if slot.d_dep is not None else None,
                                                       y_map, x_map, y_arr, x_arr, self.ds.min_depth, self.ds.max_depth)
        slot.consumed = torch.cuda.Event()
        slot.consumed.record(cur)
        inputs = {'seg': seg}
        if dep is not None:
            inputs['depth'], inputs['depth_mask'] = dep, msk
        s = [self.ds.samples[i] for i in slot.indices]
        meta = {k: [e[k] for e in s] for k in ('city', 'seq', 'frame', 'target_frame')}
        meta['start_frame'] = [e['start_fr'] for e in s]
        return {'inputs': inputs, 'labels': {'seg': lab}, 'meta': meta}

    def batches(self, epoch):
        plan = self.index_batches(epoch)
        if not plan:
            return
        self._setup()
        director = ThreadPoolExecutor(1)        # runs decode(k + 1) (which fans out to the pool) beside the consumer of batch k
        try:
            pending = director.submit(self.decode, self._slots[0], plan[0], epoch)
            for k in range(len(plan)):
                slot = self._slots[k % 2]
                pending.result()
                self.upload(slot)
                if k + 1 < len(plan):
                    nxt = self._slots[(k + 1) % 2]
                    nxt.uploaded.synchronize()      # its staging was last read by the upload of batch k - 1
                    pending = director.submit(self.decode, nxt, plan[k + 1], epoch)
                yield self.augment(slot)
        finally:
            director.shutdown(wait=True)

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
