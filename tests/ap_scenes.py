"""Seeded scenes for the instance-AP tests: ground-truth instance maps made of runs (instances, groups, void, small regions) and
prediction masks of chosen overlap.  ``hand_scene`` is written out pixel by pixel so that every rule of the definition is met by a
known prediction; ``random_scene`` fills any shape."""
import os

import numpy as np

INSTANCE_LABELS = (24, 25, 26, 27, 28, 31, 32, 33)
ROAD = 7


def _flat(n, fill):
    return np.full(n, fill, np.int64)


def hand_scene():
    """Three 40x60 images.  Returns (masks [P,H,W] u8, mask_image [P], labels [P], scores [P], gt [3,H,W] int64, notes) where
    notes maps a name to the index of the prediction that plays that part.  Image 0 holds every rule, image 1 has ground truth
    and no prediction, image 2 a prediction and no ground truth."""
    h, w = 40, 60
    n = h * w
    gt = [_flat(n, ROAD) for _ in range(3)]
    masks, image, labels, scores, notes = [], [], [], [], {}

    def pred(name, img, label, conf, ranges, value=255):
        m = np.zeros(n, np.uint8)
        for s, e in ranges:
            m[s:e] = value
        notes[name] = len(masks)
        masks.append(m.reshape(h, w))
        image.append(img)
        labels.append(label)
        scores.append(conf)

    g = gt[0]
    g[0:300] = 26001                                   # a car of 300 pixels
    pred('exact', 0, 26, 0.9, [(0, 300)])
    pred('duplicate', 0, 26, 0.8, [(0, 200)], value=1)              # 200 / 300: a second hit on the car up to t = 0.65
    g[300:500] = 24                                    # a group of persons
    pred('hits group', 0, 24, 0.7, [(300, 480)])       # 180 / 200 = 0.9: dropped while it hits, and by its ignore share after
    g[500:550] = 25001                                 # a rider of 50 pixels: small at min_region 100
    pred('hits small', 0, 25, 0.6, [(500, 550)])
    g[600:800] = 0                                     # void
    pred('void just below', 0, 26, 0.5, [(600, 700), (1000, 1101)])     # 100 / 201 <= 0.5: a false positive at every threshold
    pred('void just above', 0, 26, 0.45, [(700, 800), (1101, 1200)])    # 100 / 199 > 0.5: dropped at t = 0.5 only
    g[1200:1210] = 33                                  # a small group of bicycles: its intersection counts twice below min_region
    pred('small group', 0, 33, 0.4, [(1200, 1225)])    # ignore 20 / 25 at min_region 100, 10 / 25 at min_region 3
    g[1300:1400] = 32001
    pred('exactly 0.5', 0, 32, 0.95, [(1300, 1350)])   # 50 / 100: no hit at t = 0.5, > is strict
    g[1400:1500] = 32002
    pred('exactly 0.75', 0, 32, 0.85, [(1400, 1475)])
    g[1500:1600] = 28001
    pred('exactly 3/5', 0, 28, 0.75, [(1500, 1560)])   # 0.6 is not above 0.6000000000000001
    pred('empty', 0, 26, 0.99, [])
    pred('stuff label', 0, 7, 0.99, [(2000, 2100)])
    pred('caravan label', 0, 29, 0.99, [(2100, 2200)])
    g[1700:1702] = 27001                               # a truck of 2 pixels: regular at min_region 1 only
    pred('tiny', 0, 27, 0.65, [(1700, 1702)])
    g[1800:1850] = 29001                               # a caravan: neither void nor an instance class
    g[1850:1900] = 14                                  # guard rail: void
    pred('mixed', 0, 26, 0.35, [(250, 320), (1800, 1900)])     # 50 of the car, 20 of the person group (another label), caravan, void
    gt[1][100:400] = 26002                             # image 1: a car nobody predicts and a train: a class with gt and no prediction
    gt[1][500:650] = 31001
    pred('no ground truth', 2, 26, 0.3, [(10, 200)])   # image 2 is all road
    return (np.stack(masks), np.array(image, np.int32), np.array(labels, np.int32), np.array(scores, np.float64),
            np.stack([x.reshape(h, w) for x in gt]), notes)


def per_image(masks, mask_image, labels, scores, gt):
    """The scene as the restatement takes it: [(masks, labels, scores, gt)] per image."""
    out = []
    for i in range(len(gt)):
        sel = np.nonzero(np.asarray(mask_image) == i)[0]
        out.append((masks[sel], np.asarray(labels)[sel], np.asarray(scores)[sel], gt[i]))
    return out


def random_scene(shape, seed, n_masks):
    """gt [B,H,W] int64 of runs and n_masks predictions (masks u8, mask_image int32 unsorted, labels int32, scores float64)."""
    b, h, w = shape
    n = h * w
    rng = np.random.default_rng(seed)
    gt = np.empty((b, n), np.int64)
    pool = []
    for i in range(b):
        values = [ROAD, ROAD, 0, 3, 14, 21, 29001, 30, 1000, 23999]
        for label in rng.choice(INSTANCE_LABELS, size=5):
            values += [int(label) * 1000 + int(k) for k in rng.choice([0, 1, 2, 5, 17, 999], size=2, replace=False)]
            values.append(int(label))
        pos = 0
        while pos < n:
            run = int(min(n - pos, max(1, rng.geometric(1.0 / max(2.0, n / 40.0)))))
            gt[i, pos:pos + run] = values[int(rng.integers(len(values)))]
            pos += run
        pool.append(values)
    masks = np.zeros((n_masks, n), np.uint8)
    image = rng.integers(0, b, size=n_masks).astype(np.int32) if b else np.zeros(n_masks, np.int32)
    labels = np.empty(n_masks, np.int32)
    for k in range(n_masks):
        things = pool[image[k]][10:]                                     # the instances and groups of the image
        target = things[int(rng.integers(len(things)))]
        labels[k] = target if target < 1000 else target // 1000
        kind = k % 6
        if kind == 5:
            labels[k] = int(rng.choice([7, 29, 0, 23]))                 # not an instance class
        if kind == 4:
            continue                                                     # an empty mask
        m = gt[image[k]] == target
        if kind in (1, 2):                                               # lose a stretch, gain another
            s = int(rng.integers(0, n))
            m[s:s + max(1, n // 7)] = False
            s = int(rng.integers(0, n))
            m[s:s + max(1, n // (9 if kind == 1 else 3))] = True
        if kind == 3:
            m = rng.random(n) < 0.3
        masks[k] = np.where(m, rng.choice([1, 255, 7]), 0)
    scores = np.round(rng.random(n_masks), 1) + 0.05                    # few distinct values: equal confidences happen
    return gt.reshape(b, h, w), masks.reshape(n_masks, h, w), image, labels, scores.astype(np.float64)


def write_tree(root, masks, mask_image, labels, scores, gt, names=None):
    """A gtFine/<split> tree with *_gtFine_instanceIds.png (16-bit) and a prediction folder for it in the 'cityscapes' format (one
    txt per image, mask PNGs under masks/).  Returns (gt folder, prediction folder, stems)."""
    from PIL import Image
    gt_dir, pred_dir = os.path.join(root, 'gtFine', 'val'), os.path.join(root, 'pred')
    os.makedirs(os.path.join(pred_dir, 'masks'), exist_ok=True)
    stems = []
    for i in range(len(gt)):
        city = 'aachen' if i % 2 == 0 else 'bonn'
        stem = names[i] if names else '%s_%06d_%06d' % (city, i, 19)
        os.makedirs(os.path.join(gt_dir, city), exist_ok=True)
        Image.fromarray(gt[i].astype(np.uint16)).save(os.path.join(gt_dir, city, stem + '_gtFine_instanceIds.png'))
        lines = []
        for k in np.nonzero(np.asarray(mask_image) == i)[0]:
            rel = 'masks/%s_%03d.png' % (stem, k)
            Image.fromarray(np.where(masks[k] != 0, 255, 0).astype(np.uint8)).save(os.path.join(pred_dir, rel))
            lines.append('%s %d %r\n' % (rel, int(labels[k]), float(scores[k])))
        with open(os.path.join(pred_dir, stem + '.txt'), 'w') as f:
            f.writelines(lines)
        stems.append(stem)
    return gt_dir, pred_dir, stems


def write_panoptic(root, seg, stems):
    """The folder export_panoptic.py writes, from seg [B,H,W] of labelId * 1000 + id values: R + 256 G + 65536 B."""
    from PIL import Image
    out = os.path.join(root, 'panoptic')
    os.makedirs(out, exist_ok=True)
    for i, stem in enumerate(stems):
        ids = seg[i].astype(np.int64)
        rgb = np.stack([ids % 256, ids // 256 % 256, ids // 65536], -1).astype(np.uint8)
        Image.fromarray(rgb).save(os.path.join(out, stem + '_pred_panoptic.png'))
    return out
