#!/usr/bin/env python
"""Semantic (pixel-level) evaluation driver: IoU per class and mIoU of a tree of label PNGs against the ground truth.

    python -u panoptic-forecasting_amd/eval_semantic.py --gt-folder GT --prediction-folder PRED \\
        [--results_file OUT.json] [--format cityscapes|trainid] [--matcher device|host] [--batch_size 8] [--num_workers 8]

in place of ``cityscapesscripts.evaluation.evalPixelLevelSemanticLabeling``, to which the reference leaves this step.  That package
is absent here and its version unpinned: the formula (``semantic_iou.iou_from_confusion``) is written down from that evaluator as
remembered; parity unpinned.  iIoU is not computed.

``GT`` is a ``gtFine/<split>`` tree: ``<city>/*_gtFine_labelIds.png`` (``--format cityscapes``, the default) or
``<city>/*_labelTrainIds.png`` (``--format trainid``).  ``PRED`` is the tree ``export_bg.py`` / ``export_semantic.py`` write, with the
same relative names; images are paired by relative path.  (A ``--no_convert`` export holds trainIds under the ``..._labelIds.png``
name: with ``--format trainid`` a prediction missing under the ground truth's name is looked for under that one.)  A ground-truth
file without a prediction, a shape mismatch and a map that is not 8-bit single-channel are errors naming the file.

The PNGs are read on a thread pool and go to the device as bytes through pinned staging; ``semantic_iou.SemanticIoU`` counts them
there (``--matcher device``, batches stay in flight: ``update`` only enqueues) or ``semantic_iou.confusion_host`` on the host
(``--matcher host``).  Under an initialised process group the images are sharded round-robin and the int64 tables gathered
(``eval_panoptic.gather_total``: device tensors under RCCL); rank 0 writes the file (All / Stuff / MO / per_class / pixel_acc as fractions and the
[20,20] table under 'confusion'; an absent class's iou is ``null``) and prints the table.
"""
import argparse
import glob
import json
import math
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

from . import dist as pfdist       # noqa: E402
from . import hop_io               # noqa: E402
from . import semantic_iou         # noqa: E402
from .eval_panoptic import EvalError, LABEL_NAMES, N_CLS, gather_total  # noqa: E402

GT_SUFFIX = {'cityscapes': '_gtFine_labelIds.png', 'trainid': '_labelTrainIds.png'}
SPLITS = ('All', 'Stuff', 'MO')


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--gt-folder', dest='gt_folder', required=True)
    ap.add_argument('--prediction-folder', dest='prediction_folder', required=True)
    ap.add_argument('--results_file', default='resultPixelLevelSemanticLabeling.json')
    ap.add_argument('--format', dest='format', choices=('cityscapes', 'trainid'), default='cityscapes')
    ap.add_argument('--matcher', choices=('device', 'host'), default='device')
    ap.add_argument('--batch_size', type=int, default=8)
    ap.add_argument('--num_workers', type=int, default=8)
    return ap.parse_args(argv)


def pair_images(a):
    """[(relative name, gt png, prediction png)] in sorted ground-truth order."""
    suffix = GT_SUFFIX[a.format]
    found = sorted(glob.glob(os.path.join(a.gt_folder, '*', '*' + suffix)))
    if not found:
        raise EvalError('no ground truth <city>/*%s under %s' % (suffix, a.gt_folder))
    pairs = []
    for gf in found:
        rel = os.path.relpath(gf, a.gt_folder)
        names = [rel]
        if a.format == 'trainid':                 # a --no_convert export: trainIds under the export's own file name
            names.append(rel[:-len(suffix)] + ('' if rel.endswith('_gtFine' + suffix) else '_gtFine') + '_labelIds.png')
        pf = next((p for p in (os.path.join(a.prediction_folder, n) for n in names) if os.path.isfile(p)), None)
        if pf is None:
            raise EvalError('no prediction for ground-truth image %s in %s' % (rel, a.prediction_folder))
        pairs.append((rel, gf, pf))
    return pairs


def read_pair(item):
    rel, gf, pf = item
    g, p = hop_io.read_png(gf), hop_io.read_png(pf)
    for arr, path in ((g, gf), (p, pf)):
        if arr.ndim != 2 or arr.dtype != np.uint8:
            raise EvalError('image %s: %s is not an 8-bit single-channel label PNG' % (rel, path))
    if g.shape != p.shape:
        raise EvalError('image %s: ground truth is %dx%d, prediction %dx%d' % ((rel,) + g.shape + p.shape))
    return g, p


def _bytes_on_device(arr, device):
    """[B,H,W] u8 host array -> the same bytes on the device (pinned staging, asynchronous copy)."""
    t = torch.from_numpy(arr)
    if torch.cuda.is_available():
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


def accumulate(pairs, a, device=None):
    """[20,20] int64 confusion table of this rank's images (device matcher: on the device)."""
    if a.matcher == 'device':
        device = device or torch.device('cuda', torch.cuda.current_device())
        meter = semantic_iou.SemanticIoU(N_CLS, fmt=a.format, device=device)
    acc = torch.zeros(semantic_iou.N_CELLS, semantic_iou.N_CELLS, dtype=torch.int64)
    with ThreadPoolExecutor(max_workers=max(1, a.num_workers)) as pool:
        loaded = pool.map(read_pair, pairs)
        batch, shape = [], None
        def flush():
            if not batch:
                return
            g = np.stack([x[0] for x in batch])
            p = np.stack([x[1] for x in batch])
            if a.matcher == 'device':
                meter.update(_bytes_on_device(p, device), _bytes_on_device(g, device))
            else:
                semantic_iou.confusion_host(torch.from_numpy(p), torch.from_numpy(g), N_CLS, fmt=a.format, acc=acc)
            del batch[:]
        for g, p in loaded:
            if batch and (g.shape != shape or len(batch) >= a.batch_size):
                flush()
            shape = g.shape
            batch.append((g, p))
        flush()
    if a.matcher == 'device':
        meter.result()                                    # waits; raises on a set status word
        acc = meter.acc
    return acc


def results_from_acc(acc, names=LABEL_NAMES):
    """The file's content: All / Stuff / MO {'miou','n'} and pixel_acc as fractions, per_class by label name (None = absent)."""
    s = semantic_iou.iou_from_confusion(acc, scale=1.0)
    clean = lambda x: None if math.isnan(x) else x
    out = {k: {'miou': clean(s[k]['miou']), 'n': s[k]['n']} for k in SPLITS}
    out['per_class'] = {names[c]: clean(s['per_class'][c]) for c in range(len(names))}
    out['pixel_acc'] = clean(s['pixel_acc'])
    out['confusion'] = torch.as_tensor(acc).cpu().tolist()
    return out


def print_table(res, out=None):
    out = out or sys.stdout
    pct = lambda x: '%7s' % 'nan' if x is None else '%7.2f' % (100 * x)
    out.write('%-16s %7s %4s\n' % ('', 'IoU', 'N'))
    for name, iou in res['per_class'].items():
        out.write('%-16s %s\n' % (name, pct(iou)))
    out.write('-' * 30 + '\n')
    for name in SPLITS:
        out.write('%-16s %s %4d\n' % (name, pct(res[name]['miou']), res[name]['n']))
    out.write('%-16s %s\n' % ('pixel accuracy', pct(res['pixel_acc'])))


def run(a):
    rank, world = (torch.distributed.get_rank(), torch.distributed.get_world_size()) if pfdist.is_dist() else (0, 1)
    pairs = pair_images(a)
    if a.matcher == 'device' and not torch.cuda.is_available():
        raise EvalError('--matcher device needs a GPU (there is no fallback: pass --matcher host for the host path)')
    mine = [pairs[i] for i in pfdist.shard_indices(len(pairs), rank, world)]
    acc = accumulate(mine, a)
    total = gather_total(acc)
    res = results_from_acc(total)
    if rank == 0:
        with open(a.results_file, 'w', encoding='utf-8') as f:
            json.dump(res, f, indent=4)
        print_table(res)
    return res


def main(argv=None):
    a = parse_args(argv)
    pfdist.init_distributed_mode()
    try:
        run(a)
    except EvalError as e:                              # no barrier: the other ranks may not have failed
        sys.exit('eval_semantic: %s' % e)
    if pfdist.is_dist():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
