"""Independent restatement of the ground-truth preparation (include/pfhip.h, pf_gt_prepare block) in the per-segment formulation of
createPanopticImgs: np.unique, one boolean mask per id, mask.sum(), column and row sums for the box.  No code of the package; its own
copy of the label facts it needs (the public Cityscapes table)."""
import numpy as np

#            id: (trainId, hasInstances, ignoreInEval)
LABEL_FACTS = {0: (255, 0, 1), 1: (255, 0, 1), 2: (255, 0, 1), 3: (255, 0, 1), 4: (255, 0, 1), 5: (255, 0, 1), 6: (255, 0, 1),
               7: (0, 0, 0), 8: (1, 0, 0), 9: (255, 0, 1), 10: (255, 0, 1), 11: (2, 0, 0), 12: (3, 0, 0), 13: (4, 0, 0),
               14: (255, 0, 1), 15: (255, 0, 1), 16: (255, 0, 1), 17: (5, 0, 0), 18: (255, 0, 1), 19: (6, 0, 0), 20: (7, 0, 0),
               21: (8, 0, 0), 22: (9, 0, 0), 23: (10, 0, 0), 24: (11, 1, 0), 25: (12, 1, 0), 26: (13, 1, 0), 27: (14, 1, 0),
               28: (15, 1, 0), 29: (255, 1, 1), 30: (255, 1, 1), 31: (16, 1, 0), 32: (17, 1, 0), 33: (18, 1, 0)}


def legal(v):
    return 0 <= v < 34 or 1000 <= v < 34000


def label_of(v):
    return v if v < 1000 else v // 1000


def prepare_image(inst):
    """One [H,W] map of Python-int-valued pixels -> dict: 'flagged' (an illegal value), 'rgb' [H,W,3] u8, 'train' [H,W] u8, 'nofg'
    [H,W] u8, 'rows' [[v, area, x, y, width, height]] in ascending v, 'info' the original's segment dicts.  The pixel outputs of an
    illegal value are void (black, 255); a flagged image lists nothing."""
    inst = np.asarray(inst).astype(np.int64)
    h, w = inst.shape
    rgb = np.zeros((h, w, 3), np.uint8)
    train = np.full((h, w), 255, np.uint8)
    nofg = np.full((h, w), 255, np.uint8)
    rows, info, flagged = [], [], False
    for v in np.unique(inst).tolist():
        mask = inst == v
        if not legal(v):
            flagged = True
            continue
        train_id, has_instances, ignore = LABEL_FACTS[label_of(v)]
        train[mask] = train_id
        nofg[mask] = 255 if (has_instances and not ignore) else train_id
        if ignore:
            continue
        rgb[mask] = (v % 256, v // 256 % 256, v // 65536)
        area = int(mask.sum())
        hor_idx = np.nonzero(mask.sum(axis=0))[0]
        x = int(hor_idx[0])
        width = int(hor_idx[-1]) - x + 1
        vert_idx = np.nonzero(mask.sum(axis=1))[0]
        y = int(vert_idx[0])
        height = int(vert_idx[-1]) - y + 1
        rows.append([v, area, x, y, width, height])
        info.append({'id': v, 'category_id': label_of(v), 'area': area, 'bbox': [x, y, width, height],
                     'iscrowd': int(v < 1000 and bool(has_instances))})
    if flagged:
        rows, info = [], []
    return {'flagged': flagged, 'rgb': rgb, 'train': train, 'nofg': nofg, 'rows': rows, 'info': info}


def prepare(insts):
    return [prepare_image(m) for m in insts]
