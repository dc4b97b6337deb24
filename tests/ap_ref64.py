"""Instance AP restated in plain Python loops, in the shape of the original evaluator (evalInstanceLevelSemanticLabeling as
remembered: parity unpinned): every prediction keeps the full list of ground-truth regions it touches (matchedGt), every region the
full list of predictions touching it (matchedPred), and the lists of every class and threshold are built from those.  No `best`
shortcut, no import of instance_ap, no device."""
import numpy as np

INSTANCE_LABELS = (24, 25, 26, 27, 28, 31, 32, 33)
CLASS_NAMES = ('person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle')
VOID_IDS = (0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30)
OVERLAPS = np.arange(0.5, 1.0, 0.05)


def assign(masks, labels, scores, gt):
    """One image: masks [P,H,W], labels, scores, gt [H,W] -> (gts per label, preds per label) with the cross lists."""
    gt = np.asarray(gt).astype(np.int64)
    gts = {l: [] for l in INSTANCE_LABELS}
    for v in np.unique(gt).tolist():
        label = v if v < 1000 else v // 1000
        if label in gts:
            gts[label].append({'instID': v, 'pixelCount': int((gt == v).sum()), 'matchedPred': []})
    void = np.isin(gt, VOID_IDS)
    preds = {l: [] for l in INSTANCE_LABELS}
    for m, label, conf in zip(masks, labels, scores):
        label = int(label)
        if label not in preds:
            continue
        m = np.asarray(m) != 0
        count = int(m.sum())
        if count == 0:
            continue
        pred = {'pixelCount': count, 'confidence': float(conf), 'voidIntersection': int((m & void).sum()), 'matchedGt': []}
        for g in gts[label]:
            inter = int((m & (gt == g['instID'])).sum())
            if inter > 0:
                pred['matchedGt'].append({'instID': g['instID'], 'pixelCount': g['pixelCount'], 'intersection': inter})
                g['matchedPred'].append({'pixelCount': count, 'confidence': float(conf), 'intersection': inter})
        preds[label].append(pred)
    return gts, preds


def curve(y_true, y_score, hard_fn):
    if len(y_score) == 0:
        return 0.0                                    # every prediction dropped: the original would raise
    y_true, y_score = np.array(y_true, np.float64), np.array(y_score, np.float64)
    order = np.argsort(y_score)
    ys, yt = y_score[order], y_true[order]
    cum = np.cumsum(yt)
    _, first = np.unique(ys, return_index=True)
    n, n_true = len(ys), cum[-1]
    cum = np.append(cum, 0)
    precision, recall = np.zeros(len(first) + 1), np.zeros(len(first) + 1)
    for k, idx in enumerate(first):
        c = cum[idx - 1]
        tp = n_true - c
        fp = n - idx - tp
        fn = c + hard_fn
        precision[k] = float(tp) / (tp + fp)
        recall[k] = float(tp) / (tp + fn)
    precision[-1], recall[-1] = 1.0, 0.0
    r = np.append(np.append(recall[0], recall), 0.0)
    return float(np.dot(precision, np.convolve(r, [-0.5, 0, 0.5], 'valid')))


def evaluate(images, min_region=100):
    """images: [(masks [P,H,W], labels [P], scores [P], gt [H,W])].  Returns {'lists': {(class, threshold index): (sorted
    (true, score) pairs, hard_fn)}, 'ap' [8][10], 'classes', 'allAp', 'allAp50%'}."""
    matches = [assign(*img) for img in images]
    ap = np.full((len(INSTANCE_LABELS), len(OVERLAPS)), np.nan)
    lists = {}
    for ti, th in enumerate(OVERLAPS):
        for ci, label in enumerate(INSTANCE_LABELS):
            y_true, y_score, hard_fn = [], [], 0
            have_gt = have_pred = False
            for gts, preds in matches:
                regular = [g for g in gts[label] if g['instID'] >= 1000 and g['pixelCount'] >= min_region]
                have_gt = have_gt or bool(regular)
                have_pred = have_pred or bool(preds[label])
                cur_true, cur_score, cur_match = [1] * len(regular), [-np.inf] * len(regular), [False] * len(regular)
                for gi, g in enumerate(regular):
                    found = False
                    for pr in g['matchedPred']:
                        overlap = float(pr['intersection']) / (g['pixelCount'] + pr['pixelCount'] - pr['intersection'])
                        if overlap > th:
                            conf = pr['confidence']
                            if cur_match[gi]:
                                hi, lo = max(cur_score[gi], conf), min(cur_score[gi], conf)
                                cur_score[gi] = hi
                                cur_true.append(0)
                                cur_score.append(lo)
                                cur_match.append(True)
                            else:
                                found = True
                                cur_match[gi] = True
                                cur_score[gi] = conf
                    if not found:
                        hard_fn += 1
                for t, s, m in zip(cur_true, cur_score, cur_match):
                    if m:
                        y_true.append(t)
                        y_score.append(s)
                for pr in preds[label]:
                    found = False
                    for g in pr['matchedGt']:
                        overlap = float(g['intersection']) / (g['pixelCount'] + pr['pixelCount'] - g['intersection'])
                        if overlap > th:
                            found = True
                            break
                    if not found:
                        ignore = pr['voidIntersection']
                        for g in pr['matchedGt']:
                            if g['instID'] < 1000:
                                ignore += g['intersection']
                            if g['pixelCount'] < min_region:
                                ignore += g['intersection']
                        if float(ignore) / pr['pixelCount'] <= th:
                            y_true.append(0)
                            y_score.append(pr['confidence'])
            lists[(ci, ti)] = (sorted(zip(y_true, y_score)), hard_fn)
            if have_gt and have_pred:
                ap[ci, ti] = curve(y_true, y_score, hard_fn)
            elif have_gt:
                ap[ci, ti] = 0.0

    def nanmean(x):
        x = [float(v) for v in np.ravel(x) if not np.isnan(v)]
        return sum(x) / len(x) if x else float('nan')

    return {'lists': lists, 'ap': ap.tolist(),
            'classes': {CLASS_NAMES[c]: {'ap': nanmean(ap[c]), 'ap50%': float(ap[c, 0])} for c in range(len(INSTANCE_LABELS))},
            'allAp': nanmean(ap), 'allAp50%': nanmean(ap[:, 0])}
