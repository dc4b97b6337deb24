"""Independent restatement of the instance-weighted sums behind iIoU (include/pfhip.h, pf_iiou_accumulate block) and of
semantic_iou.iiou_from_sums / category_scores, in numpy masks and Python ints and floats: no code of the package, its own id
and size tables.

    an instance of an image: a distinct value v > 1000 of its instance map (always labelIds: label = v // 1000, k = v % 1000)
    it counts when its label has a trainId c with 11 <= c < n_cls; everything else is ignored
    size = its pixels; tp = those whose prediction is c (trainid) / the label (cityscapes)
    w = AVG[c] / size; itp += tp * w; ifn += (size - tp) * w, per image and class in ascending v from 0.0
"""
import numpy as np

TRAINID_OF_LABEL = {24: 11, 25: 12, 26: 13, 27: 14, 28: 15, 31: 16, 32: 17, 33: 18}
AVG = {11: 3462.4756337644, 12: 3930.4788056518, 13: 12794.0202738185, 14: 27855.1264367816, 15: 35732.1511111111,
       16: 67422.8757396450, 17: 6298.7200839748, 18: 4672.3249222261}
CATEGORY_CLASSES = {'flat': [0, 1], 'construction': [2, 3, 4], 'object': [5, 6, 7], 'nature': [8, 9], 'sky': [10], 'human': [11, 12],
                    'vehicle': [13, 14, 15, 16, 17, 18]}
NAN = float('nan')


def image_terms(pred, inst, n_cls=19, fmt='trainid', descending=False):
    """One image -> ([8][2] Python floats, [8][3] Python ints)."""
    pred, inst = np.asarray(pred), np.asarray(inst)
    if (pred < 0).any() or (pred > 255).any() or (inst < 0).any() or (inst > 65535).any():
        raise ValueError('value out of range')
    sums = [[0.0, 0.0] for _ in range(8)]
    counts = [[0, 0, 0] for _ in range(8)]
    values = [int(v) for v in np.unique(inst) if v > 1000]          # ascending
    for v in (values[::-1] if descending else values):
        label = v // 1000
        c = TRAINID_OF_LABEL.get(label)
        if c is None or c >= n_cls:
            continue
        mask = inst == v
        size = int(np.count_nonzero(mask))
        tp = int(np.count_nonzero(mask & (pred == (c if fmt == 'trainid' else label))))
        w = AVG[c] / float(size)
        sums[c - 11][0] = sums[c - 11][0] + float(tp) * w
        sums[c - 11][1] = sums[c - 11][1] + float(size - tp) * w
        counts[c - 11][0] += 1
        counts[c - 11][1] += size
        counts[c - 11][2] += tp
    return sums, counts


def instance_sums(pred, inst, n_cls=19, fmt='trainid', descending=False):
    """pred, inst [B,H,W] -> (per_image [B,8,2] float64, per_image_counts [B,8,3] int64)."""
    pred, inst = np.asarray(pred), np.asarray(inst)
    out = [image_terms(pred[b], inst[b], n_cls, fmt, descending) for b in range(pred.shape[0])]
    return (np.array([s for s, _ in out], np.float64).reshape(-1, 8, 2), np.array([c for _, c in out], np.int64).reshape(-1, 8, 3))


def running_sum(per_image):
    """[N,8,2] -> [8,2]: the pairs added image by image from 0.0, as a meter adds them."""
    total = [[0.0, 0.0] for _ in range(8)]
    for img in np.asarray(per_image).tolist():
        for t in range(8):
            total[t][0] = total[t][0] + img[t][0]
            total[t][1] = total[t][1] + img[t][1]
    return np.array(total, np.float64)


def _ints(table):
    return [[int(x) for x in row] for row in np.asarray(table)]


def iiou(table, sums, scale=100.0):
    """{'miou','n','per_class' (8, nan = absent)}: itp / (itp + fp + ifn), fp = the unweighted false positives of the table."""
    t, s = _ints(table), np.asarray(sums).tolist()
    per = []
    for k in range(8):
        c = 11 + k
        fp = sum(t[g][c] for g in range(19)) - t[c][c]
        d = s[k][0] + fp + s[k][1]
        per.append(scale * (s[k][0] / d) if d > 0 else NAN)
    have = [x for x in per if x == x]
    return {'miou': sum(have) / len(have) if have else NAN, 'n': len(have), 'per_class': per}


def categories(table, sums=None, scale=100.0):
    """{'per_category': {name: {'iou','iiou'}}, 'iou': {'miou','n'}, 'iiou': {'miou','n'}}."""
    t = _ints(table)
    s = np.asarray(sums).tolist() if sums is not None else None
    per = {}
    for name, members in CATEGORY_CLASSES.items():
        tp = sum(t[g][p] for g in members for p in members)
        fn = sum(sum(t[g]) for g in members) - tp
        fp = sum(t[g][p] for g in range(19) if g not in members for p in members)
        d = tp + fp + fn
        entry = {'iou': scale * (tp / d) if d else NAN, 'iiou': NAN}
        if s is not None and name in ('human', 'vehicle'):
            itp = ifn = 0.0
            for c in members:
                itp, ifn = itp + s[c - 11][0], ifn + s[c - 11][1]
            di = itp + fp + ifn
            entry['iiou'] = scale * (itp / di) if di > 0 else NAN
        per[name] = entry
    out = {'per_category': per}
    for key in ('iou', 'iiou'):
        have = [e[key] for e in per.values() if e[key] == e[key]]
        out[key] = {'miou': sum(have) / len(have) if have else NAN, 'n': len(have)}
    return out
