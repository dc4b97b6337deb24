"""Label maps and PNG trees for the semantic IoU tests and tools/bench_miou.py: the panoptic test scenes (tests/pq_scenes.py)
reduced to classes."""
import os

import numpy as np

import conf_ref64 as C
import pq_scenes as S


def to_classes(ids):
    """Panoptic trainId-format values -> trainIds: an instance value c * 1000 + k becomes c; 255 (void) stays."""
    ids = np.asarray(ids)
    return np.where(ids >= 1000, ids // 1000, ids)


def make_scenes(n=6, h=64, w=128, seed=7):
    """(pred, gt) [n,h,w] int64 trainId maps with void (255) in both."""
    preds, gts = S.make_scenes(n=n, h=h, w=w, seed=seed)
    return to_classes(preds), to_classes(gts)


def random_maps(shape, seed, fmt='trainid'):
    """Uniformly random maps over every class and a few void values: no runs at all."""
    rng = np.random.default_rng(seed)
    pool = np.array(list(range(19)) + [255, 19, 34, 200]) if fmt == 'trainid' else np.array(list(C.ID_OF_TRAINID.values()) + [0, 1, 6, 34, 255])
    return pool[rng.integers(0, len(pool), shape)], pool[rng.integers(0, len(pool), shape)]


def write_tree(root, preds, gts, fmt='cityscapes', export_names=False):
    """<root>/gt/<city>/..., <root>/pred/<city>/... from trainId maps; returns the driver's folder and format flags.
    cityscapes: labelIds under *_gtFine_labelIds.png.  trainid: *_gtFine_labelTrainIds.png; with export_names the predictions carry
    the name a --no_convert export gives them (*_gtFine_labelIds.png)."""
    from PIL import Image
    for kind, maps in (('gt', gts), ('pred', preds)):
        for i, m in enumerate(maps):
            city = 'city%d' % (i % 2)
            os.makedirs(os.path.join(root, kind, city), exist_ok=True)
            arr = C.to_cityscapes(m) if fmt == 'cityscapes' else np.asarray(m)
            suffix = '_gtFine_labelIds.png' if fmt == 'cityscapes' or (export_names and kind == 'pred') else '_gtFine_labelTrainIds.png'
            Image.fromarray(arr.astype(np.uint8)).save(os.path.join(root, kind, city, '%s_%06d_000019%s' % (city, i, suffix)))
    return ['--gt-folder', os.path.join(root, 'gt'), '--prediction-folder', os.path.join(root, 'pred'), '--format', fmt]


def run_maps(shape, seed, change=0.08):
    """Maps made of runs a dozen pixels long on average (independent in pred and gt), over every class and a few void values:
    runs end inside a lane's 16 bytes, between lanes and across rows."""
    rng = np.random.default_rng(seed)
    pool = np.array(list(range(19)) + [255, 19, 200])
    n = int(np.prod(shape))
    out = []
    for _ in range(2):
        values = pool[rng.integers(0, len(pool), n)]
        out.append(values[np.cumsum(rng.random(n) < change)].reshape(shape))
    return out[0], out[1]
