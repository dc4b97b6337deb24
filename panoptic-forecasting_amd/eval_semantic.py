#!/usr/bin/env python
"""Semantic (pixel-level) evaluation driver: IoU and iIoU per class, category scores and mIoU of a tree of label PNGs.

    python -u panoptic-forecasting_amd/eval_semantic.py --gt-folder GT --prediction-folder PRED \\
        [--results_file OUT.json] [--format cityscapes|trainid] [--matcher device|host] [--instances auto|require|off]
        [--batch_size 8] [--num_workers 8]

in place of ``cityscapesscripts.evaluation.evalPixelLevelSemanticLabeling``, to which the reference leaves this step.  That package
is absent here and its version unpinned: the formula (``semantic_iou.iou_from_confusion``) is written down from that evaluator as
remembered; parity unpinned.  So are iIoU and the category scores.

``GT`` is a ``gtFine/<split>`` tree: ``<city>/*_gtFine_labelIds.png`` (``--format cityscapes``, the default) or
``<city>/*_labelTrainIds.png`` (``--format trainid``).  ``PRED`` is the tree ``export_bg.py`` / ``export_semantic.py`` write, with the
same relative names; images are paired by relative path.  (A ``--no_convert`` export holds trainIds under the ``..._labelIds.png``
name: with ``--format trainid`` a prediction missing under the ground truth's name is looked for under that one.)  A ground-truth
file without a prediction, a shape mismatch and a map that is not 8-bit single-channel are errors naming the file.

Instances: the instance map of a ground-truth image is its name with the label suffix (``_labelIds.png`` / ``_labelTrainIds.png``)
replaced by ``_instanceIds.png``: a single-channel 16-bit or 32-bit PNG of the ground truth's shape, always in labelIds
(``labelId * 1000 + k``).  ``--instances auto`` (the default) uses them when every ground-truth image has one and none when no image
has one (a mixture is an error naming the first missing file), ``require`` makes a missing file an error, ``off`` ignores them.
Without instances the file and the table are the ones of a run before iIoU existed, key for key.  With them the file gains 'iIoU'
(mean, n, per_class), 'instances' (count and pixels per class) and 'categories' (iou / iiou per category and their means), the
table an iIoU column and the category block.  The float64 instance sums keep one order whatever the world size: every rank keeps
its images' [8,2] pairs, they are gathered by global index and added in sorted ground-truth order.

The PNGs are read on a thread pool and go to the device as bytes through pinned staging; ``semantic_iou.SemanticIoU`` counts them
there (``--matcher device``, batches stay in flight: ``update`` only enqueues) or ``semantic_iou.confusion_host`` on the host
(``--matcher host``).  Under an initialised process group the images are sharded round-robin and the int64 tables gathered
(``eval_common.gather_total``: device tensors under RCCL); rank 0 writes the file (All / Stuff / MO / per_class / pixel_acc as fractions and the
[20,20] table under 'confusion'; an absent class's iou is ``null``) and prints the table.
"""
import argparse
import glob
import math
import os
import sys

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
from . import eval_common          # noqa: E402
from .eval_common import EvalError, LABEL_NAMES, N_CLS, gather_total  # noqa: E402

GT_SUFFIX = {'cityscapes': '_gtFine_labelIds.png', 'trainid': '_labelTrainIds.png'}
LABEL_SUFFIX = {'cityscapes': '_labelIds.png', 'trainid': '_labelTrainIds.png'}      # what _instanceIds.png replaces
INSTANCE_SUFFIX = '_instanceIds.png'
THING_NAMES = LABEL_NAMES[semantic_iou.FIRST_MO:]
SPLITS = ('All', 'Stuff', 'MO')


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--gt-folder', dest='gt_folder', required=True)
    ap.add_argument('--prediction-folder', dest='prediction_folder', required=True)
    ap.add_argument('--results_file', default='resultPixelLevelSemanticLabeling.json')
    ap.add_argument('--format', dest='format', choices=('cityscapes', 'trainid'), default='cityscapes')
    ap.add_argument('--matcher', choices=('device', 'host'), default='device')
    ap.add_argument('--instances', choices=('auto', 'require', 'off'), default='auto')
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


def with_instances(pairs, a):
    """The pairs with their instance PNG as a fourth element, or the pairs as they are when the run has no instances."""
    if a.instances == 'off':
        return pairs
    files = [gf[:-len(LABEL_SUFFIX[a.format])] + INSTANCE_SUFFIX for _, gf, _ in pairs]
    have = [os.path.isfile(f) for f in files]
    if a.instances == 'auto' and not any(have):
        return pairs
    if not all(have):
        missing = files[have.index(False)]
        raise EvalError('no instance map %s (--instances %s: %d of %d ground-truth images have one)'
                        % (missing, a.instances, sum(have), len(have)))
    return [pair + (f,) for pair, f in zip(pairs, files)]


def read_pair(item):
    rel, gf, pf = item[:3]
    g, p = hop_io.read_png(gf), hop_io.read_png(pf)
    for arr, path in ((g, gf), (p, pf)):
        if arr.ndim != 2 or arr.dtype != np.uint8:
            raise EvalError('image %s: %s is not an 8-bit single-channel label PNG' % (rel, path))
    if g.shape != p.shape:
        raise EvalError('image %s: ground truth is %dx%d, prediction %dx%d' % ((rel,) + g.shape + p.shape))
    if len(item) == 3:
        return g, p
    i = hop_io.read_png(item[3])
    if i.ndim != 2 or i.dtype.kind not in 'iu' or i.dtype.itemsize not in (2, 4):
        raise EvalError('image %s: %s is not a single-channel 16-bit or 32-bit instance PNG' % (rel, item[3]))
    if i.shape != g.shape:
        raise EvalError('image %s: ground truth is %dx%d, instance map %s %dx%d' % ((rel,) + g.shape + (item[3],) + i.shape))
    return g, p, (i.view(np.int16) if i.dtype.itemsize == 2 else i.astype(np.int32, copy=False))   # 16-bit stays 16-bit


def accumulate(pairs, a, device=None, inst_out=None):
    """[20,20] int64 confusion table of this rank's images (device matcher: on the device).  Where the pairs carry instance files
    (with_instances), the dict ``inst_out`` receives 'per_image' ([n,8,2] float64, the images' (itp, ifn) pairs in the order of
    ``pairs``) and 'counts' ([8,3] int64), both on the host."""
    n_things = semantic_iou.N_THINGS
    if a.matcher == 'device':
        device = device or torch.device('cuda', torch.cuda.current_device())
        meter = semantic_iou.SemanticIoU(N_CLS, fmt=a.format, device=device)
    acc = torch.zeros(semantic_iou.N_CELLS, semantic_iou.N_CELLS, dtype=torch.int64)
    per_image, counts = [], torch.zeros(n_things, 3, dtype=torch.int64)
    to = eval_common.on_device
    def on_batch(g, p, i=None):
        if a.matcher == 'device':
            if i is None:
                meter.update(to(p, device), to(g, device))
            else:
                per_image.append(torch.empty(len(g), n_things, 2, dtype=torch.float64, device=device))
                meter.update(to(p, device), to(g, device), inst=to(i, device), per_image_inst=per_image[-1])
        else:
            semantic_iou.confusion_host(torch.from_numpy(p), torch.from_numpy(g), N_CLS, fmt=a.format, acc=acc)
            if i is not None:
                sums, n = semantic_iou.instance_sums_host(torch.from_numpy(p), torch.from_numpy(i), N_CLS, fmt=a.format)
                per_image.append(sums)
                counts.add_(n.sum(0))
    eval_common.for_each_batch(pairs, read_pair, a, on_batch)
    if a.matcher == 'device':
        meter.result()                                    # waits; raises on a set status word
        acc = meter.acc
        counts = meter.acc_inst_counts.cpu()
    if inst_out is not None and pairs and len(pairs[0]) == 4:
        inst_out['per_image'] = torch.cat([x.cpu() for x in per_image]) if per_image else torch.zeros(0, n_things, 2, dtype=torch.float64)
        inst_out['counts'] = counts
    return acc


def results_from_acc(acc, names=LABEL_NAMES, acc_inst=None, inst_counts=None):
    """The file's content: All / Stuff / MO {'miou','n'} and pixel_acc as fractions, per_class by label name (None = absent).
    With the instance sums also 'iIoU' {'miou','n','per_class' by label name}, 'instances' {name: {'n','pixels'}} and 'categories'
    {category: {'iou','iiou'}, 'iou': mean, 'iiou': mean}."""
    s = semantic_iou.iou_from_confusion(acc, scale=1.0)
    clean = lambda x: None if math.isnan(x) else x
    out = {k: {'miou': clean(s[k]['miou']), 'n': s[k]['n']} for k in SPLITS}
    out['per_class'] = {names[c]: clean(s['per_class'][c]) for c in range(len(names))}
    out['pixel_acc'] = clean(s['pixel_acc'])
    out['confusion'] = torch.as_tensor(acc).cpu().tolist()
    if acc_inst is not None:
        things = names[semantic_iou.FIRST_MO:]
        i = semantic_iou.iiou_from_sums(acc, acc_inst, scale=1.0)
        out['iIoU'] = {'miou': clean(i['miou']), 'n': i['n'], 'per_class': {things[t]: clean(x) for t, x in enumerate(i['per_class'])}}
        out['instances'] = {things[t]: {'n': int(row[0]), 'pixels': int(row[1])} for t, row in enumerate(torch.as_tensor(inst_counts).tolist())}
        c = semantic_iou.category_scores(acc, acc_inst, scale=1.0)
        out['categories'] = {name: {k: clean(x) for k, x in v.items()} for name, v in c['per_category'].items()}
        out['categories'].update(iou=clean(c['iou']['miou']), iiou=clean(c['iiou']['miou']))
    return out


def print_table(res, out=None):
    out = out or sys.stdout
    pct = lambda x: '%7s' % 'nan' if x is None else '%7.2f' % (100 * x)
    if 'iIoU' not in res:
        out.write('%-16s %7s %4s\n' % ('', 'IoU', 'N'))
        for name, iou in res['per_class'].items():
            out.write('%-16s %s\n' % (name, pct(iou)))
        out.write('-' * 30 + '\n')
        for name in SPLITS:
            out.write('%-16s %s %4d\n' % (name, pct(res[name]['miou']), res[name]['n']))
        out.write('%-16s %s\n' % ('pixel accuracy', pct(res['pixel_acc'])))
        return
    blank = '%7s' % ''
    out.write('%-16s %7s %7s %4s\n' % ('', 'IoU', 'iIoU', 'N'))
    for name, iou in res['per_class'].items():
        out.write('%-16s %s %s\n' % (name, pct(iou), pct(res['iIoU']['per_class'][name]) if name in res['iIoU']['per_class'] else blank))
    out.write('-' * 38 + '\n')
    for name in SPLITS:
        out.write('%-16s %s %s %4d\n' % (name, pct(res[name]['miou']), pct(res['iIoU']['miou']) if name == 'MO' else blank, res[name]['n']))
    out.write('%-16s %s\n' % ('pixel accuracy', pct(res['pixel_acc'])))
    out.write('-' * 38 + '\n')
    for name, _ in semantic_iou.CATEGORIES:
        c = res['categories'][name]
        out.write('%-16s %s %s\n' % (name, pct(c['iou']), pct(c['iiou']) if c['iiou'] is not None else blank))
    out.write('%-16s %s %s\n' % ('categories', pct(res['categories']['iou']), pct(res['categories']['iiou'])))


def ordered_instance_sums(per_image, n_images, world):
    """This rank's [n,8,2] float64 per-image pairs (image r, r + world, ... of the sorted list) -> the [8,2] sums over all images,
    added in sorted ground-truth order from 0.0: one order, hence one result, for every world size.  The pairs travel as they are
    (128 B per image, padded to the longest shard) and are put back by global index."""
    slots = (n_images + world - 1) // world
    mine = torch.zeros(slots, semantic_iou.N_THINGS, 2, dtype=torch.float64)
    mine[:len(per_image)] = per_image
    if pfdist.is_dist() and str(torch.distributed.get_backend()) != 'gloo':
        mine = mine.to(torch.device('cuda', torch.cuda.current_device()))
    everyone = pfdist.gather_accumulators(mine).cpu()              # [world, slots, 8, 2]
    total = torch.zeros(semantic_iou.N_THINGS, 2, dtype=torch.float64)
    for i in range(n_images):
        total += everyone[i % world, i // world]
    return total


def run(a):
    rank, world = eval_common.rank_world()
    pairs = pair_images(a)
    eval_common.require_matcher(a)
    pairs = with_instances(pairs, a)
    mine = [pairs[i] for i in pfdist.shard_indices(len(pairs), rank, world)]
    if len(pairs[0]) == 3:
        res = results_from_acc(gather_total(accumulate(mine, a)))
    else:
        sums = {'per_image': torch.zeros(0, semantic_iou.N_THINGS, 2, dtype=torch.float64),
                'counts': torch.zeros(semantic_iou.N_THINGS, 3, dtype=torch.int64)}
        acc = accumulate(mine, a, inst_out=sums)
        total, counts = gather_total(acc), gather_total(sums['counts'])
        res = results_from_acc(total, acc_inst=ordered_instance_sums(sums['per_image'], len(pairs), world), inst_counts=counts)
    return eval_common.write_results(res, a, print_table)


def main(argv=None):
    eval_common.main('eval_semantic', parse_args, run, argv)


if __name__ == '__main__':
    main()
