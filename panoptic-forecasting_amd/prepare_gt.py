#!/usr/bin/env python
"""Cityscapes ground-truth preparation driver - the three commands of the reference's README (data preparation), from a raw
``gtFine`` download and nothing else:

    python -u panoptic-forecasting_amd/prepare_gt.py panoptic --dataset-folder GTFINE [--output-folder DIR]
        [--set-names val train test] [--use-train-id]
    python -u panoptic-forecasting_amd/prepare_gt.py trainids --dataset-folder GTFINE [--set-names ...]
    python -u panoptic-forecasting_amd/prepare_gt.py remove_fg --input_dir GTFINE/train --output_dir NOFG/train
    python -u panoptic-forecasting_amd/prepare_gt.py all --dataset-folder GTFINE --nofg-output NOFG [--output-folder DIR] ...

each with ``[--backend device|host] [--batch_size 8] [--num_workers 8]``.

``panoptic`` stands in for ``python -m cityscapesscripts.preparation.createPanopticImgs`` and takes its flags.  It writes
``<out>/cityscapes_panoptic_<set>[_trainId]/<name>_gtFine_panoptic.png`` and ``<out>/cityscapes_panoptic_<set>[_trainId].json``
(``<out>`` defaults to the dataset folder): {"images": [{"id", "width", "height", "file_name": <name>_gtFine_leftImg8bit.png}],
"annotations": [{"image_id", "file_name", "segments_info": [{"id", "category_id", "area", "bbox": [x, y, w, h], "iscrowd"}]}],
"categories": [{"id", "name", "color", "supercategory", "isthing"}]}, images in sorted file order - the ``--gt-folder`` and
``--gt-json-file`` of eval_panoptic.py.  That package is absent here and its version unpinned: this layout is written down from the
original as remembered; layout and parity unpinned.

``trainids`` stands in for ``createTrainIdLabelImgs``: it writes ``*_gtFine_labelTrainIds.png`` beside each instance map.  The
original rasterises the polygon file with trainIds; the rasteriser is not rebuilt here.  ``*_labelIds.png`` and
``*_instanceIds.png`` of the download are rasterised from the same polygons in the same order, a pixel of the instance map holds its
labelId (below 1000) or labelId * 1000 + index, and trainId is a function of labelId alone: looking the labelId of every instance-map
pixel up gives the map the original draws.

``remove_fg`` takes the two flags of the reference's ``scripts/preprocessing/remove_fg_from_gt.py`` and reads
``<input_dir>/<city>/*_gtFine_labelTrainIds.png``; it is bound by PNG decoding and always runs its 256-entry table on the host.
``all`` decodes each instance map once, makes one device call per batch and writes all three outputs, the last under
``<nofg-output>/<set>/<city>/`` (the ``data.gt_dir`` of bg training).

The PNGs are read and written on thread pools; with ``--backend device`` a batch's call and download are enqueued before the
previous batch's files are written, and a batch is finished by waiting for its own event; an illegal value is refused naming the
first and last file of its batch.  Existing outputs are overwritten.  A set without instance maps is reported by name and
skipped.  One process only.
"""
import argparse
import glob
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if __package__ in (None, ''):                     # run as a script: make the package importable under its alias
    sys.path.insert(0, os.path.dirname(_HERE))
    import panoptic_forecasting_amd  # noqa: F401
    __package__ = 'panoptic_forecasting_amd'

from . import eval_common          # noqa: E402
from . import gt_prep              # noqa: E402
from . import hop_io               # noqa: E402
from . import lib as _lib          # noqa: E402
from .eval_common import EvalError  # noqa: E402

INSTANCE_SUFFIX = '_gtFine_instanceIds.png'
TRAINID_SUFFIX = '_gtFine_labelTrainIds.png'
PANOPTIC_SUFFIX = '_gtFine_panoptic.png'
IMAGE_SUFFIX = '_gtFine_leftImg8bit.png'
WANT = {'panoptic': ('panoptic',), 'trainids': ('trainids',), 'all': ('panoptic', 'trainids', 'nofg')}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='command', required=True)

    def common(p):
        p.add_argument('--backend', choices=('device', 'host'), default='device')
        p.add_argument('--batch_size', type=int, default=8)
        p.add_argument('--num_workers', type=int, default=8)

    def dataset(p):
        p.add_argument('--dataset-folder', dest='dataset_folder', required=True, help='the gtFine folder')
        p.add_argument('--set-names', dest='set_names', nargs='+', default=['val', 'train', 'test'])

    def panoptic(p):
        p.add_argument('--output-folder', dest='output_folder', default=None, help='default: the dataset folder')
        p.add_argument('--use-train-id', dest='use_train_id', action='store_true')

    p = sub.add_parser('panoptic')
    dataset(p), panoptic(p), common(p)
    p = sub.add_parser('trainids')
    dataset(p), common(p)
    p = sub.add_parser('remove_fg')
    p.add_argument('--input_dir', required=True)
    p.add_argument('--output_dir', required=True)
    common(p)
    p = sub.add_parser('all')
    dataset(p), panoptic(p), common(p)
    p.add_argument('--nofg-output', dest='nofg_output', required=True)
    return ap.parse_args(argv)


def read_instances(path):
    arr = hop_io.read_png(path)
    if arr.ndim != 2 or arr.dtype.kind not in 'iu' or arr.dtype.itemsize not in (2, 4):
        raise EvalError('%s is not a single-channel 16-bit or 32-bit instance PNG' % path)
    return (arr.view(np.int16) if arr.dtype.itemsize == 2 else arr.astype(np.int32, copy=False),)   # 16-bit stays 16-bit


class Writer:
    """What one set's batches become: files, written on a pool of their own, and the JSON's entries by image index."""

    def __init__(self, a, set_name, files):
        self.a, self.set_name, self.files = a, set_name, files
        self.want = WANT[a.command]
        self.pool = ThreadPoolExecutor(max_workers=max(1, a.num_workers))
        self.jobs = []
        self.images, self.annotations = [None] * len(files), [None] * len(files)
        self.pan_dir = None
        if 'panoptic' in self.want:
            out = a.output_folder or a.dataset_folder
            self.pan_name = 'cityscapes_panoptic_%s%s' % (set_name, '_trainId' if a.use_train_id else '')
            self.pan_dir = os.path.join(out, self.pan_name)
            os.makedirs(self.pan_dir, exist_ok=True)

    def _write(self, path, arr):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        hop_io.write_png(path, arr)

    def emit(self, first, res):
        """Images first .. of the set from one batch's host arrays."""
        rows = gt_prep.segment_rows(res) if 'panoptic' in self.want else None
        for b in range(len(next(iter(res.values())))):
            path = self.files[first + b]
            city, base = os.path.basename(os.path.dirname(path)), os.path.basename(path)[:-len(INSTANCE_SUFFIX)]
            if 'panoptic' in self.want:
                h, w = res['panoptic'].shape[1:3]
                self.images[first + b] = {'id': base, 'width': int(w), 'height': int(h), 'file_name': base + IMAGE_SUFFIX}
                self.annotations[first + b] = {'image_id': base, 'file_name': base + PANOPTIC_SUFFIX,
                                               'segments_info': gt_prep.segments_info(rows[b], self.a.use_train_id)}
                self.jobs.append(self.pool.submit(self._write, os.path.join(self.pan_dir, base + PANOPTIC_SUFFIX), res['panoptic'][b]))
            if 'trainids' in self.want:
                self.jobs.append(self.pool.submit(self._write, path[:-len(INSTANCE_SUFFIX)] + TRAINID_SUFFIX, res['trainids'][b]))
            if 'nofg' in self.want:
                self.jobs.append(self.pool.submit(self._write, os.path.join(self.a.nofg_output, self.set_name, city, base + TRAINID_SUFFIX),
                                                  res['nofg'][b]))

    def close(self):
        for job in self.jobs:
            job.result()
        self.pool.shutdown()
        if self.pan_dir is not None:
            doc = {'images': self.images, 'annotations': self.annotations, 'categories': gt_prep.categories(self.a.use_train_id)}
            with open(self.pan_dir + '.json', 'w', encoding='utf-8') as f:
                json.dump(doc, f, indent=4)


def prepare_set(a, set_name, files, preparer):
    writer = Writer(a, set_name, files)
    state = {'next': 0, 'pending': None}

    def refuse(first, count, e):
        return EvalError('set %s, images %s .. %s: %s' % (set_name, files[first], os.path.basename(files[first + count - 1]), e))

    def finish(pending):
        """Waits for one batch's own event - not for what was enqueued behind it - and reads the status word copied behind its call."""
        first, count, host, word, event = pending
        event.synchronize()
        try:
            preparer.raise_for(int(word[0]))
        except _lib.PfError as e:
            raise refuse(first, count, e)
        writer.emit(first, {k: v.numpy() for k, v in host.items()})

    def on_batch(inst):
        first = state['next']
        state['next'] += len(inst)
        if preparer is None:
            try:
                writer.emit(first, gt_prep.prepare_host(inst, writer.want))
            except _lib.PfError as e:
                raise refuse(first, len(inst), e)
            return
        res = preparer.prepare(eval_common.on_device(inst, preparer.device), writer.want, check=False)
        host = {k: torch.empty(v.shape, dtype=v.dtype, pin_memory=True).copy_(v, non_blocking=True) for k, v in res.items()}
        word = preparer.status_async()
        event = torch.cuda.Event()
        event.record()
        previous, state['pending'] = state['pending'], (first, len(inst), host, word, event)
        if previous is not None:
            finish(previous)

    eval_common.for_each_batch(files, read_instances, a, on_batch)
    if state['pending'] is not None:
        finish(state['pending'])
    writer.close()


def run_remove_fg(a):
    def one(item):
        src, dst = item
        seg = hop_io.read_png(src)
        if seg.ndim != 2 or seg.dtype != np.uint8:
            raise EvalError('%s is not an 8-bit single-channel trainId PNG' % src)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        hop_io.write_png(dst, gt_prep.remove_fg_host(seg))
    if not os.path.isdir(a.input_dir):
        raise EvalError('no input folder %s' % a.input_dir)
    items = []
    for city in sorted(os.listdir(a.input_dir)):
        for src in sorted(glob.glob(os.path.join(a.input_dir, city, '*' + TRAINID_SUFFIX))):
            items.append((src, os.path.join(a.output_dir, city, os.path.basename(src))))
    if not items:
        print('prepare_gt: no <city>/*%s under %s: nothing written' % (TRAINID_SUFFIX, a.input_dir))
    with ThreadPoolExecutor(max_workers=max(1, a.num_workers)) as pool:
        list(pool.map(one, items))
    return len(items)


def run(a):
    if a.command == 'remove_fg':
        return run_remove_fg(a)
    preparer = None
    if a.backend == 'device':
        if not torch.cuda.is_available():
            raise EvalError('--backend device needs a GPU (there is no fallback: pass --backend host for the host path)')
        preparer = gt_prep.GTPreparer(torch.device('cuda', torch.cuda.current_device()))
    done = 0
    for set_name in a.set_names:
        files = sorted(glob.glob(os.path.join(a.dataset_folder, set_name, '*', '*' + INSTANCE_SUFFIX)))
        if not files:
            print('prepare_gt: set %s: no <city>/*%s under %s: skipped' % (set_name, INSTANCE_SUFFIX, os.path.join(a.dataset_folder, set_name)))
            continue
        prepare_set(a, set_name, files, preparer)
        print('prepare_gt: set %s: %d images' % (set_name, len(files)))
        done += len(files)
    return done


def main(argv=None):
    a = parse_args(argv)
    try:
        run(a)
    except EvalError as e:
        sys.exit('prepare_gt: %s' % e)


if __name__ == '__main__':
    main()
