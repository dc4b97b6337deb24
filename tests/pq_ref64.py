"""Panoptic quality restated in numpy and plain Python: the reference of tests/test_pq_host.py and tests/test_gpu_pq.py.

Independent of panoptic_forecasting_amd.pq and of the HIP kernels: no torch, no hashing - dicts over np.unique of the (gt, pred)
pairs.  Semantics (include/pfhip.h, pf_pq_accumulate):
  * category of a value v: v // 1000 for v >= 1000, else v; 'trainid' format: that is the trainId (void 255 is no class),
    'cityscapes' format: a Cityscapes id, mapped back to its trainId (void 0 is no class).  A category that is none of the n_cls
    classes is void; void is ONE pseudo-segment, every other segment is its raw value.
  * crowd (when switched on): a ground-truth value < 1000 of a thing class (trainId 11..18).
  * TP: gt not void / crowd, same category, inter / (g_area + p_area - inter - p_void[p]) > 0.5 in float64.
  * FN: gt not void / crowd, unmatched.  FP: pred not void, unmatched, unless p_void + p_crowd(same category) > p_area / 2.
IoUs are added per class in ascending (image, gt id) order.
"""
import numpy as np

TRAINID2ID = (7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33)
FIRST_THING = 11
VOID = 'void'


def to_cityscapes(m):
    """A trainId-format map (void 255) in Cityscapes ids (void 0): what the panoptic export writes."""
    m = np.asarray(m).astype(np.int64)
    out = np.zeros_like(m)
    table = np.array(TRAINID2ID, dtype=np.int64)
    stuff = (m < 19)
    out[stuff] = table[m[stuff]]
    thing = (m >= 1000) & (m // 1000 < 19)
    out[thing] = table[m[thing] // 1000] * 1000 + m[thing] % 1000
    return out


def category(v, fmt, n_cls):
    base = v // 1000 if v >= 1000 else v
    if fmt == 'trainid':
        t = base
    elif fmt == 'cityscapes':
        t = TRAINID2ID.index(base) if base in TRAINID2ID else -1
    else:
        raise ValueError(fmt)
    return t if 0 <= t < n_cls else -1


def image_matches(pred, gt, n_cls=19, fmt='trainid', crowd=True):
    """One image -> (tp [(class, gt id, iou)] in ascending gt id, fp [n_cls] int, fn [n_cls] int, excused: how many unmatched
    predictions were not counted as FP)."""
    p = np.asarray(pred).astype(np.int64).ravel()
    g = np.asarray(gt).astype(np.int64).ravel()
    if p.size and (min(p.min(), g.min()) < 0 or max(p.max(), g.max()) > 65535):
        raise ValueError('label value outside [0, 65536)')
    pairs, counts = np.unique(np.stack([g, p], 1), axis=0, return_counts=True)
    g_area, p_area, p_void, p_crowd, inter = {}, {}, {}, {}, {}
    cat = {}
    for (gv, pv), n in zip(pairs.tolist(), counts.tolist()):
        gc, pc = category(gv, fmt, n_cls), category(pv, fmt, n_cls)
        gk = VOID if gc < 0 else gv
        pk = VOID if pc < 0 else pv
        cat[('g', gk)], cat[('p', pk)] = gc, pc
        g_area[gk] = g_area.get(gk, 0) + n
        p_area[pk] = p_area.get(pk, 0) + n
        inter[(gk, pk)] = inter.get((gk, pk), 0) + n
        if gk == VOID:
            p_void[pk] = p_void.get(pk, 0) + n
        elif crowd and gv < 1000 and gc >= FIRST_THING and gc == pc:
            p_crowd[pk] = p_crowd.get(pk, 0) + n
    is_crowd = lambda gk: crowd and gk != VOID and gk < 1000 and cat[('g', gk)] >= FIRST_THING
    g_keys = sorted(k for k in g_area if k != VOID and not is_crowd(k))
    p_keys = sorted(k for k in p_area if k != VOID)
    tp, g_hit, p_hit = [], set(), set()
    for gk in g_keys:
        for pk in p_keys:
            n = inter.get((gk, pk), 0)
            if not n or cat[('g', gk)] != cat[('p', pk)]:
                continue
            iou = np.float64(n) / np.float64(g_area[gk] + p_area[pk] - n - p_void.get(pk, 0))
            if iou > 0.5:
                assert gk not in g_hit and pk not in p_hit
                tp.append((cat[('g', gk)], gk, float(iou)))
                g_hit.add(gk)
                p_hit.add(pk)
    fp, fn, excused = [0] * n_cls, [0] * n_cls, 0
    for gk in g_keys:
        if gk not in g_hit:
            fn[cat[('g', gk)]] += 1
    for pk in p_keys:
        if pk in p_hit:
            continue
        if 2 * (p_void.get(pk, 0) + p_crowd.get(pk, 0)) > p_area[pk]:
            excused += 1
        else:
            fp[cat[('p', pk)]] += 1
    return tp, fp, fn, excused


def accumulate(preds, gts, n_cls=19, fmt='trainid', crowd=True):
    """[B,H,W] maps -> (acc [n_cls,4] float64, per_image [B,n_cls,4] float64, excused)."""
    acc = np.zeros((n_cls, 4), np.float64)
    per_image = np.zeros((len(preds), n_cls, 4), np.float64)
    excused = 0
    for b in range(len(preds)):
        tp, fp, fn, ex = image_matches(preds[b], gts[b], n_cls, fmt, crowd)
        excused += ex
        for c, _, iou in tp:
            acc[c, 0] += iou
            acc[c, 1] += 1
            per_image[b, c, 0] += iou
            per_image[b, c, 1] += 1
        for c in range(n_cls):
            acc[c, 2] += fp[c]
            acc[c, 3] += fn[c]
            per_image[b, c, 2] = fp[c]
            per_image[b, c, 3] = fn[c]
    return acc, per_image, excused


def splits(acc, scale=100.0):
    """{'All','Things','Stuff'} -> {'pq','sq','rq','n'} and per_class [{'pq','sq','rq'}]."""
    rows = []
    for siou, tp, fp, fn in np.asarray(acc, np.float64).tolist():
        d = tp + 0.5 * fp + 0.5 * fn
        rows.append(None if d <= 0 else (siou / d, siou / tp if tp > 0 else 0.0, tp / d))
    out = {}
    for name, sel in (('All', range(len(rows))), ('Things', range(FIRST_THING, len(rows))), ('Stuff', range(min(FIRST_THING, len(rows))))):
        have = [rows[c] for c in sel if rows[c] is not None]
        d = max(len(have), 1)
        out[name] = {'pq': scale * sum(r[0] for r in have) / d, 'sq': scale * sum(r[1] for r in have) / d,
                     'rq': scale * sum(r[2] for r in have) / d, 'n': len(have)}
    out['per_class'] = [{'pq': 0.0, 'sq': 0.0, 'rq': 0.0} if r is None else {'pq': scale * r[0], 'sq': scale * r[1], 'rq': scale * r[2]}
                        for r in rows]
    return out
