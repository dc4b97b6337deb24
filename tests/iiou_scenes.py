"""Predictions, ground truth and instance maps for the iIoU tests and tools/bench_iiou.py: the panoptic test scenes
(tests/pq_scenes.py) with their ground truth written as a Cityscapes instance map (labelId * 1000 + k for a thing instance, the
labelId for stuff and for a thing group, 0 for void), and maps made of runs over a pool of instance values."""
import os

import numpy as np

import conf_ref64 as C
import conf_scenes as CS
import pq_scenes as S

THING_LABELS = (24, 25, 26, 27, 28, 31, 32, 33)
# every thing class at the first, the last and two more indices; stuff; a car group; caravan and trailer instances (not evaluated);
# 1000 and 1001 (label 1: not an instance / no trainId); void; a label past the table; the largest u16
INST_POOL = np.array([l * 1000 + k for l in THING_LABELS for k in (0, 1, 2, 999)] + [7, 8, 11, 21, 23, 26, 29001, 30002, 1000, 1001, 0,
                                                                                    34005, 65535])
PRED_POOL = np.array(list(range(19)) + list(range(11, 19)) * 2 + [255, 19, 200])


def to_instance_map(ids):
    """Panoptic trainId-format values (c * 1000 + k, c, 255) -> a Cityscapes instance map."""
    ids = np.asarray(ids)
    out = np.zeros(ids.shape, np.int64)
    for t, label in C.ID_OF_TRAINID.items():
        out[ids == t] = label
        thing = (ids >= 1000) & (ids // 1000 == t)
        out[thing] = label * 1000 + ids[thing] % 1000
    return out


def make_scenes(n=6, h=64, w=128, seed=7):
    """(pred, gt, inst) [n,h,w] int64: trainId maps with void (255) in both, and the ground truth's instance map."""
    preds, gts = S.make_scenes(n=n, h=h, w=w, seed=seed)
    return CS.to_classes(preds), CS.to_classes(gts), to_instance_map(gts)


def inst_run_maps(shape, seed, change=0.08):
    """(pred trainIds, inst) made of runs a dozen pixels long on average, independent of one another: runs end inside a lane's
    load, between lanes and across rows; the instance values come from INST_POOL."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    out = []
    for pool in (PRED_POOL, INST_POOL):
        values = pool[rng.integers(0, len(pool), n)]
        out.append(values[np.cumsum(rng.random(n) < change)].reshape(shape).astype(np.int64))
    return out[0], out[1]


def many_persons(seed, n_inst=240, h=96, w=160):
    """One image (pred, inst) [1,h,w] with n_inst person instances of differing sizes laid out in runs, about half of each hit."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 101, n_inst)
    sizes = sizes[np.cumsum(sizes) <= h * w]
    inst = np.full(h * w, 7, np.int64)
    pred = np.zeros(h * w, np.int64)
    at = 0
    for k, s in enumerate(sizes.tolist()):
        inst[at:at + s] = 24000 + k + 1
        pred[at:at + int(rng.integers(0, s + 1))] = 11
        at += s
    return pred.reshape(1, h, w), inst.reshape(1, h, w)


def in_format(pred, fmt):
    return C.to_cityscapes(pred) if fmt == 'cityscapes' else np.asarray(pred)


def write_tree(root, preds, gts, insts, fmt='cityscapes', only=None, bits=16):
    """conf_scenes.write_tree plus <root>/gt/<city>/*_gtFine_instanceIds.png for the images in ``only`` (default: all)."""
    from PIL import Image
    flags = CS.write_tree(root, preds, gts, fmt)
    for i, m in enumerate(insts):
        if only is not None and i not in only:
            continue
        city = 'city%d' % (i % 2)
        arr = np.asarray(m).astype(np.uint16 if bits == 16 else np.int32)
        Image.fromarray(arr).save(os.path.join(root, 'gt', city, '%s_%06d_000019_gtFine_instanceIds.png' % (city, i)))
    return flags


def instance_file(root, i):
    city = 'city%d' % (i % 2)
    return os.path.join(root, 'gt', city, '%s_%06d_000019_gtFine_instanceIds.png' % (city, i))
