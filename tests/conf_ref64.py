"""Independent restatement of the semantic confusion table and of IoU / mIoU (include/pfhip.h, pf_confusion_accumulate block;
semantic_iou.iou_from_confusion), in numpy and Python floats: a double loop over the classes with boolean masks - no bincount, no
code of the package, its own id table.

    table[g, p] = number of pixels whose ground truth has class g and whose prediction has class p; index 19 = void
    trainid:     values 0..18 are classes, everything else void      cityscapes: labelIds, ID_OF_TRAINID inverted, the rest void
    a class >= n_cls is void
"""
import numpy as np

ID_OF_TRAINID = {0: 7, 1: 8, 2: 11, 3: 12, 4: 13, 5: 17, 6: 19, 7: 20, 8: 21, 9: 22, 10: 23, 11: 24, 12: 25, 13: 26, 14: 27, 15: 28,
                 16: 31, 17: 32, 18: 33}
VOID = 19
STUFF = range(0, 11)
MOVING = range(11, 19)


def class_mask(values, c, n_cls, fmt):
    """Boolean mask of the pixels of class c (0..18), or of void for c == 19."""
    values = np.asarray(values)
    if (values < 0).any() or (values > 255).any():
        raise ValueError('label value outside [0, 256)')
    if c != VOID:
        if c >= n_cls:
            return np.zeros(values.shape, bool)
        return values == (c if fmt == 'trainid' else ID_OF_TRAINID[c])
    void = np.ones(values.shape, bool)
    for k in range(n_cls):
        void &= ~class_mask(values, k, n_cls, fmt)
    return void


def confusion(pred, gt, n_cls=19, fmt='trainid'):
    """pred, gt [B,H,W] -> (table [20,20] int64, per_image [B,20,20] int64)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    per = np.zeros((pred.shape[0], 20, 20), np.int64)
    for b in range(pred.shape[0]):
        pm = [class_mask(pred[b], c, n_cls, fmt) for c in range(20)]
        for g in range(20):
            gm = class_mask(gt[b], g, n_cls, fmt)
            if not gm.any():
                continue
            for p in range(20):
                per[b, g, p] = int(np.count_nonzero(gm & pm[p]))
    return per.sum(0), per


def to_cityscapes(ids):
    """trainId map (anything else = void) -> labelIds, void -> 0."""
    ids = np.asarray(ids)
    out = np.zeros(ids.shape, ids.dtype)
    for t, i in ID_OF_TRAINID.items():
        out[ids == t] = i
    return out


def iou(table, scale=100.0):
    """{'All','Stuff','MO'}: {'miou','n'}, 'per_class' (nan = absent), 'pixel_acc', in Python ints and floats."""
    t = [[int(x) for x in row] for row in np.asarray(table)]
    per, trace, valid = [], 0, 0
    for c in range(19):
        tp = t[c][c]
        fn = sum(t[c][p] for p in range(20)) - tp               # the void column counts: predicting void on a class is a miss
        fp = sum(t[g][c] for g in range(19)) - tp               # the void row does not: ignored ground truth excuses the prediction
        d = tp + fp + fn
        per.append(scale * (tp / d) if d else float('nan'))
        trace += tp
        valid += sum(t[c])
    out = {}
    for name, classes in (('All', range(19)), ('Stuff', STUFF), ('MO', MOVING)):
        have = [per[c] for c in classes if per[c] == per[c]]
        out[name] = {'miou': sum(have) / len(have) if have else float('nan'), 'n': len(have)}
    out['per_class'] = per
    out['pixel_acc'] = scale * (trace / valid) if valid else float('nan')
    return out
