#!/usr/bin/env python
"""Instance-level evaluation driver: AP and AP50 per thing class of predicted instance masks against ``*_gtFine_instanceIds.png``.

    python -u panoptic-forecasting_amd/eval_instances.py --gt-folder gtFine/val --prediction-folder PRED \\
        [--prediction-format cityscapes|panoptic] [--matcher device|host] [--min-region 100] [--result-file OUT.json]
        [--max-masks-per-call 64] [--batch_size 4] [--num_workers 8]

in place of ``cityscapesscripts.evaluation.evalInstanceLevelSemanticLabeling``, to which the reference leaves this step.  That
package is absent here and its version unpinned: the definition (include/pfhip.h, pf_ap_accumulate block) is written
down from that evaluator as remembered, and so is the layout of the result file: parity unpinned, both.  The distance-limited scores
(AP50m / AP100m) are not built.

``--gt-folder`` is a ``gtFine/<split>`` tree; every ``<city>/<city>_<seq>_<frame>_gtFine_instanceIds.png`` (16-bit or 32-bit,
single channel) is an image.  Predictions, by ``--prediction-format``:

  cityscapes  the instance-result format (what the reference's export_cityscapes_instance_results.py writes): one
              ``<city>_<seq>_<frame>.txt`` per image, in the prediction folder or in its ``<city>/`` folder, whose lines are
              ``mask.png labelID confidence``.  Mask paths are relative to the txt file; a path that leaves the prediction folder is
              refused.  A mask is a single-channel PNG of the image's shape, inside = non-zero.  An empty file means no predictions;
              a ground-truth image without a txt is an error naming it.
  panoptic    the folder export_panoptic.py writes (``<city>_<seq>_<frame>_pred_panoptic.png``, R + 256 G + 65536 B =
              labelId * 1000 + id for things): every thing segment is an instance of confidence 1.0
              (instance_ap.masks_from_id_map).

The PNGs are read on a thread pool.  Consecutive images of one shape form a batch of at most ``--batch_size``; its masks go to
the matcher in calls of at most ``--max-masks-per-call`` masks, which bounds the resident mask stack (an image's masks may be split
over calls).  ``--matcher device``: instance_ap.InstanceAP (csrc/ap_kernels.hip; calls stay in flight, update only enqueues);
``--matcher host``: instance_ap.records_host.  Under an initialised process group the images are sharded round-robin; every rank's
records, region counts and scores are gathered with their lengths and put in sorted ground-truth order, so the result file is
byte-identical for every world size.  Rank 0 writes it and prints the table.
"""
import argparse
import glob
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
from . import instance_ap          # noqa: E402
from . import eval_common          # noqa: E402
from . import panoptic             # noqa: E402
from .eval_common import EvalError  # noqa: E402

GT_SUFFIX = '_gtFine_instanceIds.png'
PANOPTIC_SUFFIX = '_pred_panoptic.png'


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--gt-folder', dest='gt_folder', required=True)
    ap.add_argument('--prediction-folder', dest='prediction_folder', required=True)
    ap.add_argument('--prediction-format', dest='prediction_format', choices=('cityscapes', 'panoptic'), default='cityscapes')
    ap.add_argument('--matcher', choices=('device', 'host'), default='device')
    ap.add_argument('--min-region', dest='min_region', type=int, default=instance_ap.MIN_REGION)
    ap.add_argument('--result-file', dest='results_file', default='resultInstanceLevelSemanticLabeling.json')
    ap.add_argument('--max-masks-per-call', dest='max_masks_per_call', type=int, default=64)
    ap.add_argument('--batch_size', type=int, default=4)
    ap.add_argument('--num_workers', type=int, default=8)
    a = ap.parse_args(argv)
    if a.max_masks_per_call < 1 or a.batch_size < 1 or a.min_region < 0:
        ap.error('--max-masks-per-call and --batch_size must be at least 1, --min-region not negative')
    return a


def pair_images(a):
    """[(stem, gt png, prediction file)] in sorted ground-truth order."""
    found = sorted(glob.glob(os.path.join(a.gt_folder, '*', '*' + GT_SUFFIX)))
    if not found:
        raise EvalError('no ground truth <city>/*%s under %s' % (GT_SUFFIX, a.gt_folder))
    pairs = []
    for gf in found:
        stem, city = os.path.basename(gf)[:-len(GT_SUFFIX)], os.path.basename(os.path.dirname(gf))
        name = stem + ('.txt' if a.prediction_format == 'cityscapes' else PANOPTIC_SUFFIX)
        pf = next((p for p in (os.path.join(a.prediction_folder, name), os.path.join(a.prediction_folder, city, name)) if os.path.isfile(p)), None)
        if pf is None:
            raise EvalError('no prediction %s for ground-truth image %s in %s' % (name, os.path.relpath(gf, a.gt_folder), a.prediction_folder))
        pairs.append((stem, gf, pf))
    return pairs


def read_prediction_list(txt, root):
    """[(mask png, labelId, confidence)] of one result txt; the mask paths are relative to it and stay inside ``root``."""
    out = []
    root = os.path.realpath(root)
    with open(txt, encoding='utf-8') as f:
        for n, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 3:
                raise EvalError('%s line %d: expected "mask.png labelID confidence" (got %r)' % (txt, n, line.strip()))
            try:
                label, conf = int(parts[1]), float(parts[2])
            except ValueError:
                raise EvalError('%s line %d: labelID must be an integer and confidence a number (got %r)' % (txt, n, line.strip()))
            if math.isnan(conf):
                raise EvalError('%s line %d: the confidence is not a number' % (txt, n))
            path = os.path.realpath(os.path.join(os.path.dirname(txt), parts[0]))
            if os.path.isabs(parts[0]) or os.path.commonpath([root, path]) != root:
                raise EvalError('%s line %d: mask path %s leaves the prediction folder' % (txt, n, parts[0]))
            if not os.path.isfile(path):
                raise EvalError('%s line %d: no mask file %s' % (txt, n, parts[0]))
            if not 0 <= label < instance_ap.N_LABELS:
                raise EvalError('%s line %d: labelID %d is outside [0, %d)' % (txt, n, label, instance_ap.N_LABELS))
            out.append((path, label, conf))
    return out


def make_reader(a):
    def read(item):
        """-> (gt [H,W] int16 (u16 bits) or int32, masks [p,H,W] u8, labels [p] int32, scores [p] float64)"""
        stem, gf, pf = item
        g = hop_io.read_png(gf)
        if g.ndim != 2 or g.dtype.kind not in 'iu' or g.dtype.itemsize not in (2, 4):
            raise EvalError('image %s: %s is not a single-channel 16-bit or 32-bit instance PNG' % (stem, gf))
        g = g.view(np.int16) if g.dtype.itemsize == 2 else g.astype(np.int32, copy=False)
        if a.prediction_format == 'panoptic':
            rgb = hop_io.read_png(pf)
            if rgb.ndim != 3 or rgb.shape[2] < 3 or rgb.dtype != np.uint8:
                raise EvalError('image %s: %s is not an 8-bit RGB panoptic PNG' % (stem, pf))
            if rgb.shape[:2] != g.shape:
                raise EvalError('image %s: ground truth is %dx%d, prediction %s %dx%d' % ((stem,) + g.shape + (pf,) + rgb.shape[:2]))
            masks, _, labels, scores = instance_ap.masks_from_id_map(torch.from_numpy(panoptic.decode_png(rgb[..., :3])), 'cityscapes')
            return g, masks.numpy(), labels.numpy(), scores.numpy()
        entries = read_prediction_list(pf, a.prediction_folder)
        masks = np.zeros((len(entries),) + g.shape, np.uint8)
        for k, (path, _, _) in enumerate(entries):
            m = hop_io.read_png(path)
            if m.ndim != 2:
                raise EvalError('image %s: mask %s is not a single-channel PNG' % (stem, path))
            if m.shape != g.shape:
                raise EvalError('image %s: ground truth is %dx%d, mask %s %dx%d' % ((stem,) + g.shape + (path,) + m.shape))
            masks[k] = m != 0
        return g, masks, np.array([e[1] for e in entries], np.int32), np.array([e[2] for e in entries], np.float64)
    return read


def accumulate(items, a, device=None):
    """This rank's images -> (rec [N,8] int32 whose image column counts this rank's images in order, gt_regular [n,8] int32,
    scores [N] float64), on the host."""
    if a.matcher == 'device':
        device = device or torch.device('cuda', torch.cuda.current_device())
        meter = instance_ap.InstanceAP(a.min_region, device=device)
    recs, regs, scores_out, seen = [], [], [], [0]
    to = eval_common.on_device

    def on_batch(batch):
        gt = np.stack([x[0] for x in batch])
        masks = np.concatenate([x[1] for x in batch])
        image = np.concatenate([np.full(len(x[1]), i, np.int32) for i, x in enumerate(batch)])
        labels = np.concatenate([x[2] for x in batch])
        scores = np.concatenate([x[3] for x in batch])
        g = to(gt, device) if a.matcher == 'device' else torch.from_numpy(gt)
        for call, s in enumerate(range(0, max(len(masks), 1), a.max_masks_per_call)):
            e = min(len(masks), s + a.max_masks_per_call)
            if a.matcher == 'device':
                meter.update(to(masks[s:e], device), to(image[s:e], device), to(labels[s:e], device), to(scores[s:e], device), g,
                             new_images=call == 0)
            else:
                rec, regular = instance_ap.records_host(masks[s:e], image[s:e], labels[s:e], g, a.min_region)
                rec[:, 6] += seen[0]
                recs.append(rec)
                scores_out.append(torch.from_numpy(scores[s:e]))
                if call == 0:
                    regs.append(regular)
        seen[0] += len(batch)

    with ThreadPoolExecutor(max_workers=max(1, a.num_workers)) as pool:
        batch = []
        for x in pool.map(make_reader(a), items):
            if batch and (x[0].shape != batch[0][0].shape or x[0].dtype != batch[0][0].dtype or len(batch) >= a.batch_size):
                on_batch(batch)
                batch = []
            batch.append(x)
        if batch:
            on_batch(batch)
    if a.matcher == 'device':
        meter.result()                                    # waits; raises on a set status word
        return meter.records()
    cat = lambda xs, shape, dt: torch.cat(xs) if xs else torch.zeros(shape, dtype=dt)
    return cat(recs, (0, 8), torch.int32), cat(regs, (0, instance_ap.N_CLASSES), torch.int32), cat(scores_out, (0,), torch.float64)


def gather_records(rec, regular, scores, indices, n_images):
    """Every rank's records (image column: position in ``indices``, the global numbers of its images) -> the records of all images
    in sorted ground-truth order, an image's records in the order of its file: (rec [N,8], gt_regular [n_images,8], scores [N]).
    They travel as they are, with their lengths (all_gather_object)."""
    rec = rec.clone()
    rec[:, 6] = torch.tensor(indices, dtype=torch.int32)[rec[:, 6].long()] if len(rec) else rec[:, 6]
    parts = pfdist.gather_objects((rec.numpy(), regular.numpy(), scores.numpy(), list(indices)))
    all_rec = np.concatenate([p[0] for p in parts])
    all_scores = np.concatenate([p[2] for p in parts])
    all_regular = np.zeros((n_images, instance_ap.N_CLASSES), np.int32)
    for p in parts:
        if len(p[3]):
            all_regular[np.array(p[3], np.int64)] = p[1]
    order = np.argsort(all_rec[:, 6], kind='stable')
    return all_rec[order], all_regular, all_scores[order]


def results_from_records(rec, regular, scores, a):
    """The file's content.  Its layout against the absent evaluator's is unpinned."""
    res = instance_ap.ap_from_records(rec, regular, scores, None, a.min_region)
    clean = lambda x: None if math.isnan(x) else x
    state = rec[:, 0]
    return {'averages': {'allAp': clean(res['allAp']), 'allAp50%': clean(res['allAp50%']),
                         'classes': {name: {'ap': clean(v['ap']), 'ap50%': clean(v['ap50%'])} for name, v in res['classes'].items()}},
            'thresholds': list(instance_ap.THRESHOLDS), 'min_region': a.min_region, 'images': int(len(regular)),
            'predictions': {'total': int(len(rec)), 'counted': int((state == instance_ap.COUNTED).sum()),
                            'empty': int((state == instance_ap.EMPTY).sum()),
                            'not_an_instance_class': int((state == instance_ap.NO_CLASS).sum())},
            'regular_regions': {name: int(regular[:, c].sum()) for c, name in enumerate(instance_ap.CLASS_NAMES)}}


def print_table(res, out=None):
    out = out or sys.stdout
    pct = lambda x: '%7s' % 'nan' if x is None else '%7.2f' % (100 * x)
    out.write('%-16s %7s %7s\n' % ('', 'AP', 'AP50%'))
    for name, v in res['averages']['classes'].items():
        out.write('%-16s %s %s\n' % (name, pct(v['ap']), pct(v['ap50%'])))
    out.write('-' * 32 + '\n')
    out.write('%-16s %s %s\n' % ('average', pct(res['averages']['allAp']), pct(res['averages']['allAp50%'])))
    out.write('%d images, %d predictions (%d counted), min_region %d\n'
              % (res['images'], res['predictions']['total'], res['predictions']['counted'], res['min_region']))


def run(a):
    rank, world = eval_common.rank_world()
    pairs = pair_images(a)
    eval_common.require_matcher(a)
    indices = pfdist.shard_indices(len(pairs), rank, world)
    rec, regular, scores = accumulate([pairs[i] for i in indices], a)
    rec, regular, scores = gather_records(rec, regular, scores, indices, len(pairs))
    return eval_common.write_results(results_from_records(rec, regular, scores, a), a, print_table)


def main(argv=None):
    eval_common.main('eval_instances', parse_args, run, argv)


if __name__ == '__main__':
    main()
