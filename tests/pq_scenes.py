"""Label-map scenes for the panoptic-quality tests (numpy only): the hand-made 4x8 cases, the seeded scene generator, and a
writer of the PNG + JSON tree that eval_panoptic.py reads.  All maps are made in trainId format (stuff = trainId, thing =
trainId * 1000 + instance, void 255); pq_ref64.to_cityscapes turns them into exported ids."""
import json
import os

import numpy as np

import pq_ref64 as R

# the 19 evaluated Cityscapes label names by trainId
NAMES = ('road', 'sidewalk', 'building', 'wall', 'fence', 'pole', 'traffic light', 'traffic sign', 'vegetation', 'terrain', 'sky',
         'person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle')


def _blank():
    return np.zeros((4, 8), np.int64), np.zeros((4, 8), np.int64)      # road everywhere: one stuff TP of IoU <= 1


def hand_scenes():
    """[(name, pred, gt, {(crowd, class): (TP, FP, FN)} expected rows)] - the numbered cases of the test plan."""
    out = []
    # 1. prediction covers exactly 2 of the 4 gt pixels and nothing else: IoU 2/4 = 0.5 is NOT a match
    p, g = _blank()
    g[0, 0:4] = 13001
    p[0, 0:2] = 13001
    out.append(('iou_half', p, g, {(True, 13): (0, 1, 1), (True, 0): (1, 0, 0)}))
    # 2. 3 of 4: IoU 0.75
    p, g = _blank()
    g[0, 0:4] = 13001
    p[0, 0:3] = 13001
    out.append(('iou_three_quarters', p, g, {(True, 13): (1, 0, 0)}))
    # 3. 6 predicted pixels: 3 on the gt segment of 4, 2 on void, 1 on road: union 4 + 6 - 3 - 2 = 5, IoU 0.6
    p, g = _blank()
    g[0, 0:4] = 13001
    g[1, 0:2] = 255
    p[0, 1:4] = 13001
    p[1, 0:3] = 13001
    out.append(('void_leaves_union', p, g, {(True, 13): (1, 0, 0)}))
    # 4. unmatched prediction, exactly half on void: FP; one pixel more on void: excused
    p, g = _blank()
    g[0, 0:2] = 255
    p[0, 0:4] = 11001
    out.append(('half_on_void', p, g, {(True, 11): (0, 1, 0)}))
    p, g = _blank()
    g[0, 0:3] = 255
    p[0, 0:4] = 11001
    out.append(('more_than_half_on_void', p, g, {(True, 11): (0, 0, 0)}))
    # 5. the same with crowd of the prediction's category (without the crowd rule value 11 is an ordinary person segment)
    p, g = _blank()
    g[0, 0:2] = 11
    p[0, 0:4] = 11001
    out.append(('half_on_crowd', p, g, {(True, 11): (0, 1, 0), (False, 11): (0, 1, 1)}))
    p, g = _blank()
    g[0, 0:3] = 11
    p[0, 0:4] = 11001
    out.append(('more_than_half_on_crowd', p, g, {(True, 11): (0, 0, 0), (False, 11): (1, 0, 0)}))
    # 6. crowd of another category excuses nothing
    p, g = _blank()
    g[0, 0:3] = 13
    p[0, 0:4] = 11001
    out.append(('crowd_of_other_category', p, g, {(True, 11): (0, 1, 0), (True, 13): (0, 0, 0), (False, 13): (0, 0, 1)}))
    # 7. a crowd segment alone: no FN (its pixels stay in road's union: 24 / 32)
    p, g = _blank()
    g[2:4, 4:8] = 13
    out.append(('crowd_alone', p, g, {(True, 13): (0, 0, 0), (False, 13): (0, 0, 1), (True, 0): (1, 0, 0)}))
    # 8. the same instance number in two categories: two segments; and a prediction of the right number in the wrong category
    p, g = _blank()
    g[0, 0:4] = 13001
    g[2, 0:4] = 14001
    p[0, 0:4] = 13001
    p[2, 0:4] = 14001
    out.append(('same_instance_two_categories', p, g, {(True, 13): (1, 0, 0), (True, 14): (1, 0, 0)}))
    p, g = _blank()
    g[0, 0:4] = 13001
    g[2, 0:4] = 14001
    p[0, 0:4] = 14001
    p[2, 0:4] = 13001
    out.append(('same_instance_wrong_category', p, g, {(True, 13): (0, 1, 1), (True, 14): (0, 1, 1)}))
    return out


def _rect(rng, h, w, min_h, max_h, min_w, max_w):
    rh, rw = int(rng.integers(min_h, max_h + 1)), int(rng.integers(min_w, max_w + 1))
    y, x = int(rng.integers(0, h - rh + 1)), int(rng.integers(0, w - rw + 1))
    return slice(y, y + rh), slice(x, x + rw)


def make_scene(rng, h=64, w=128):
    """One (pred, gt) pair.  Ground truth: three bands of stuff, small stuff rectangles, 0..12 thing instances, void and crowd
    patches.  Prediction: the ground truth shifted by a few pixels, then instances split, relabelled, dropped and invented (on
    void, on crowd of their own and of another category), and small stuff rectangles relabelled."""
    s = max(h // 64, 1)                                  # the generator scaled up keeps its proportions
    gt = np.empty((h, w), np.int64)
    bands = rng.permutation(11)[:3]
    cut1, cut2 = int(rng.integers(h // 4, h // 2)), int(rng.integers(h // 2 + 4 * s, 3 * h // 4))
    gt[:cut1], gt[cut1:cut2], gt[cut2:] = bands[0], bands[1], bands[2]
    others = [c for c in rng.permutation(11) if c not in bands]
    small = []
    for c in others[:int(rng.integers(2, 5))]:
        r = _rect(rng, h, w, 6 * s, 14 * s, 8 * s, 24 * s)
        gt[r] = c
        small.append((r, int(c)))
    things, n_inst = [], {}
    for _ in range(int(rng.integers(0, 13))):
        c = int(rng.integers(11, 19))
        r = _rect(rng, h, w, 5 * s, 18 * s, 5 * s, 22 * s)
        n_inst[c] = n_inst.get(c, 0) + 1
        gt[r] = c * 1000 + n_inst[c]
        things.append((r, c, c * 1000 + n_inst[c]))
    voids = [_rect(rng, h, w, 4 * s, 10 * s, 6 * s, 16 * s) for _ in range(int(rng.integers(1, 3)))]
    for r in voids:
        gt[r] = 255
    crowds = []
    for _ in range(int(rng.integers(0, 3))):
        c = int(rng.integers(11, 19))
        r = _rect(rng, h, w, 5 * s, 10 * s, 8 * s, 16 * s)
        gt[r] = c
        crowds.append((r, c))

    dy, dx = int(rng.integers(-2 * s, 2 * s + 1)), int(rng.integers(-3 * s, 3 * s + 1))
    pred = np.roll(gt, (dy, dx), axis=(0, 1))
    for r, c in small:                                   # a small stuff rectangle predicted as another stuff class
        if rng.random() < 0.5:
            rr = (slice(max(r[0].start + dy, 0), max(r[0].stop + dy, 0)), slice(max(r[1].start + dx, 0), max(r[1].stop + dx, 0)))
            pred[rr] = others[-1]
    next_id = {c: 500 for c in range(11, 19)}
    for r, c, v in things:
        what = rng.random()
        m = pred == v
        if not m.any():
            continue
        ys, xs = np.nonzero(m)
        if what < 0.2:                                   # split: one side keeps the id, the other becomes a new instance
            cut = xs.min() + (xs.max() - xs.min() + 1) * (0.5 if rng.random() < 0.5 else 0.25)
            next_id[c] += 1
            pred[m & (np.arange(w)[None, :] < cut)] = c * 1000 + next_id[c]
        elif what < 0.35:                                # relabelled: right place, wrong category
            c2 = 11 + (c - 11 + 1 + int(rng.integers(0, 7))) % 8
            next_id[c2] += 1
            pred[m] = c2 * 1000 + next_id[c2]
        elif what < 0.45:                                # dropped
            pred[m] = bands[1]
    for r in voids:                                      # invented on void: excused when more than half of it lies there
        if rng.random() < 0.7:
            c = int(rng.integers(11, 19))
            next_id[c] += 1
            grow = int(rng.integers(0, 3)) * s
            pred[r[0].start:r[0].stop + grow, r[1].start:r[1].stop + grow] = c * 1000 + next_id[c]
    for r, c in crowds:                                  # invented on crowd: of its category (excused) or of another (FP)
        if rng.random() < 0.8:
            c2 = c if rng.random() < 0.6 else 11 + (c - 11 + 3) % 8
            next_id[c2] += 1
            pred[r[0].start:r[0].stop, r[1].start:r[1].stop - 2 * s] = c2 * 1000 + next_id[c2]
    return pred, gt


def make_scenes(n=24, h=64, w=128, seed=2024):
    rng = np.random.default_rng(seed)
    pairs = [make_scene(rng, h, w) for _ in range(n)]
    return np.stack([p for p, _ in pairs]), np.stack([g for _, g in pairs])


def encode_rgb(ids):
    """decode_png's inverse: ids -> [H,W,3] u8 (R + 256 G + 65536 B)."""
    ids = np.asarray(ids).astype(np.int64)
    return np.stack([ids % 256, ids // 256 % 256, ids // 65536], -1).astype(np.uint8)


def segments_info(ids, with_crowd):
    info = []
    for v in np.unique(ids).tolist():
        if v == 0:
            continue
        cat = v // 1000 if v >= 1000 else v
        seg = {'id': v, 'category_id': cat}
        if with_crowd:
            seg['iscrowd'] = int(v < 1000 and cat in R.TRAINID2ID[R.FIRST_THING:])
        info.append(seg)
    return info


def write_tree(root, preds, gts, bare=False):
    """Writes <root>/gt.json + gt/, <root>/pred.json + pred/ from trainId-format maps; returns the driver's five path flags.
    bare: both JSON files are the bare list of annotations (no 'categories': the driver has to know the label names itself)."""
    from PIL import Image
    ann = {'gt': [], 'pred': []}
    for kind, maps in (('gt', gts), ('pred', preds)):
        os.makedirs(os.path.join(root, kind), exist_ok=True)
        for i, m in enumerate(maps):
            ids = R.to_cityscapes(m)
            image_id = 'synth_%06d_%06d' % (i // 4, i)
            name = image_id + ('_gtFine_panoptic.png' if kind == 'gt' else '_pred_panoptic.png')
            Image.fromarray(encode_rgb(ids)).save(os.path.join(root, kind, name))
            ann[kind].append({'image_id': image_id, 'file_name': name, 'segments_info': segments_info(ids, kind == 'gt')})
    gt_doc = {'images': [{'id': a['image_id']} for a in ann['gt']], 'annotations': ann['gt'],
              'categories': [{'id': i, 'name': n, 'isthing': int(t >= R.FIRST_THING)} for t, (i, n) in enumerate(zip(R.TRAINID2ID, NAMES))]}
    pred_doc = {'annotations': ann['pred'][::-1]}               # another order: the driver pairs by image_id
    for name, doc in (('gt.json', gt_doc), ('pred.json', pred_doc)):
        with open(os.path.join(root, name), 'w') as f:
            json.dump(doc['annotations'] if bare else doc, f)
    return ['--gt-json-file', os.path.join(root, 'gt.json'), '--gt-folder', os.path.join(root, 'gt'),
            '--prediction-json-file', os.path.join(root, 'pred.json'), '--prediction-folder', os.path.join(root, 'pred')]
