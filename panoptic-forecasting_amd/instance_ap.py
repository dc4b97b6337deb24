"""Instance AP / AP50 of predicted instance masks against a Cityscapes instance map: the semantics of include/pfhip.h's
pf_ap_accumulate block.

The reference leaves this score to the external ``cityscapesscripts.evaluation.evalInstanceLevelSemanticLabeling``; that package is
absent here and its version unpinned, so the definition is written down from that evaluator as remembered: parity unpinned
(DESIGN.md 3.17).  The distance-limited scores (AP50m / AP100m) are not built.

The work is split where the integers end.  Per prediction a *record* of eight integers
``{state, pixels, ignore, best_value, best_inter, best_pixels, image, class index}`` and per image the count of regular ground-truth
regions per class: ``InstanceAP`` enqueues the HIP kernels for them (csrc/ap_kernels.hip), ``records_host`` states the same in
torch (any device; the host path of eval_instances.py).  Everything after the records is float64 on the host and shared by both:
``ap_from_records``.  tests/ap_ref64.py restates the whole evaluation a third time, in the original's shape (full pairwise
matching), without either.

Records are integers and an image's records do not depend on its batch or on how its masks are split over calls; AP does not
depend on the order of the records.  So a sharded evaluation reproduces the single-process result bit for bit.
"""
import ctypes

import numpy as np
import torch

from .meter import DeviceMeter

INSTANCE_LABELS = (24, 25, 26, 27, 28, 31, 32, 33)              # class index 0..7; trainIds 11..18
CLASS_NAMES = ('person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle')
N_CLASSES = 8
N_LABELS = 34                                                    # a mask's labelId must be below this
THRESHOLDS = tuple(float(x) for x in np.arange(0.5, 1.0, 0.05))  # verbatim: the third is 0.6000000000000001
VOID_IDS = (0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30)  # the ignore_in_eval labels (gt_prep.LABELS; csrc/gt_labels.h)
MIN_REGION = 100
COUNTED, EMPTY, NO_CLASS, FLAGGED = 0, 1, 2, 3
STATUS_BITS = ((1, 'PF_AP_STATUS_VALUE: a ground-truth value outside [0, 65536)'),
               (2, 'PF_AP_STATUS_INDEX: a mask_image outside [0, B) or a mask_label outside [0, 34)'))
_GT_KINDS = {torch.int32: 1, torch.int64: 2}                     # any 2-byte integer tensor is read as u16: kind 0
PANOPTIC_FORMATS = ('trainid', 'cityscapes')


def class_of_label(label):
    return INSTANCE_LABELS.index(label) if label in INSTANCE_LABELS else -1


def _gt_values(gt):
    """Instance map -> int64 values; a 2-byte integer tensor is read as u16."""
    gt = torch.as_tensor(gt)
    if gt.dtype.is_floating_point or gt.dtype.is_complex or gt.dtype == torch.bool:
        raise ValueError('gt must be an integer instance map (got %s)' % gt.dtype)
    if gt.element_size() == 2:
        return gt.view(torch.int16).long() & 0xffff
    return gt.long()


def records_host(masks, mask_image, labels, gt, min_region=MIN_REGION):
    """masks [P,H,W] (inside = non-zero), mask_image [P], labels [P], gt [B,H,W] instance map, any device -> (rec [P,8] int32,
    gt_regular [B,8] int32) on the host: the records of pf_ap_accumulate stated with ``torch.bincount``.  A gt value outside
    [0, 65536), a mask_image outside [0, B) or a label outside [0, 34) is a PfError (the device flags them instead)."""
    from .lib import PfError
    masks, v = torch.as_tensor(masks), _gt_values(gt)
    mask_image = [int(x) for x in torch.as_tensor(mask_image).reshape(-1).tolist()]
    labels = [int(x) for x in torch.as_tensor(labels).reshape(-1).tolist()]
    if v.dim() != 3 or masks.dim() != 3 or tuple(masks.shape[1:]) != tuple(v.shape[1:]):
        raise ValueError('masks must be [P,H,W] and gt [B,H,W] of one image shape (got %s and %s)' % (tuple(masks.shape), tuple(v.shape)))
    p, b = masks.shape[0], v.shape[0]
    if not (len(mask_image) == len(labels) == p):
        raise ValueError('mask_image and labels must hold one entry per mask')
    if min_region < 0:
        raise ValueError('min_region must not be negative')
    if v.numel() and (int(v.min()) < 0 or int(v.max()) > 65535):
        raise PfError('PF_AP_STATUS_VALUE: a ground-truth value outside [0, 65536)')
    for i, l in zip(mask_image, labels):
        if not 0 <= i < b or not 0 <= l < N_LABELS:
            raise PfError('PF_AP_STATUS_INDEX: a mask_image outside [0, B) or a mask_label outside [0, 34) (image %d, label %d)' % (i, l))
    flat = v.reshape(b, v.shape[1] * v.shape[2])
    sizes = [torch.bincount(flat[i], minlength=65536).cpu() for i in range(b)]
    gt_regular = torch.zeros(b, N_CLASSES, dtype=torch.int32)
    for i in range(b):
        for c, label in enumerate(INSTANCE_LABELS):
            s = sizes[i][label * 1000:label * 1000 + 1000]
            gt_regular[i, c] = int(((s > 0) & (s >= min_region)).sum())
    rec = torch.zeros(p, 8, dtype=torch.int32)
    inside = masks.reshape(p, v.shape[1] * v.shape[2]) != 0
    for k in range(p):
        i, label = mask_image[k], labels[k]
        c = class_of_label(label)
        row = [COUNTED, 0, 0, -1, 0, 0, i, c]
        if c < 0:
            row[0] = NO_CLASS
        else:
            inter = torch.bincount(flat[i].to(inside.device)[inside[k]], minlength=65536).cpu()
            pixels = int(inter.sum())
            if pixels == 0:
                row[0] = EMPTY
            else:
                ignore = sum(int(inter[x]) for x in VOID_IDS)
                best = (0, -1)
                for g in [label] + list(range(label * 1000, label * 1000 + 1000)):        # ascending value: the first of equals stays
                    n = int(inter[g])
                    if n == 0:
                        continue
                    if g < 1000:
                        ignore += n
                    if int(sizes[i][g]) < min_region:
                        ignore += n
                    if n > best[0]:
                        best = (n, g)
                row[1], row[2] = pixels, ignore
                if best[1] >= 0:
                    row[3], row[4], row[5] = best[1], best[0], int(sizes[i][best[1]])
        rec[k] = torch.tensor(row, dtype=torch.int32)
    return rec, gt_regular


def average_precision(y_true, y_score, hard_fn):
    """The original's precision / recall curve from the (true, score) lists of one class and threshold and the number of regular
    regions nothing hit; float64.  An empty list (every prediction dropped) is 0.0: the original would raise there."""
    y_true, y_score = np.asarray(y_true, np.int64), np.asarray(y_score, np.float64)
    if y_score.size == 0:
        return 0.0
    order = np.argsort(y_score, kind='stable')
    y_score, y_true = y_score[order], y_true[order]
    cum = np.cumsum(y_true)
    _, first = np.unique(y_score, return_index=True)
    n, n_true = len(y_score), int(cum[-1])
    cum = np.append(cum, 0)                                       # index -1 reads 0
    precision, recall = np.zeros(len(first) + 1), np.zeros(len(first) + 1)
    for k, idx in enumerate(first):
        below = int(cum[idx - 1])
        tp = n_true - below
        fp = n - int(idx) - tp
        fn = below + hard_fn
        precision[k] = float(tp) / (tp + fp)
        recall[k] = float(tp) / (tp + fn)
    precision[-1], recall[-1] = 1.0, 0.0
    widths = np.convolve(np.concatenate([recall[:1], recall, [0.0]]), [-0.5, 0, 0.5], 'valid')
    return float(np.dot(precision, widths))


def match_lists(rec, gt_regular, scores, image_offsets=None, min_region=MIN_REGION):
    """{(class, threshold index): (y_true list, y_score list, hard_fn)} and (have_gt [8], have_pred [8]) from the records."""
    rec = np.asarray(torch.as_tensor(rec).cpu().numpy() if isinstance(rec, torch.Tensor) else rec, np.int64).reshape(-1, 8)
    regular = np.asarray(torch.as_tensor(gt_regular).cpu().numpy() if isinstance(gt_regular, torch.Tensor) else gt_regular, np.int64).reshape(-1, N_CLASSES)
    scores = np.asarray(torch.as_tensor(scores).cpu().numpy() if isinstance(scores, torch.Tensor) else scores, np.float64).reshape(-1)
    if len(scores) != len(rec):
        raise ValueError('scores must hold one confidence per record (got %d and %d)' % (len(scores), len(rec)))
    image = rec[:, 6].copy()
    if image_offsets is not None:
        image += np.broadcast_to(np.asarray(image_offsets, np.int64), image.shape)
    if (rec[:, 0] == FLAGGED).any():
        raise ValueError('a flagged record cannot be scored')
    total_regular = regular.sum(0)
    have_gt = [bool(total_regular[c] > 0) for c in range(N_CLASSES)]
    have_pred = [False] * N_CLASSES
    lists = {}
    per_class = [[] for _ in range(N_CLASSES)]
    for k in np.nonzero(rec[:, 0] == COUNTED)[0]:
        per_class[int(rec[k, 7])].append(int(k))
    for c in range(N_CLASSES):
        have_pred[c] = bool(per_class[c])
        for ti, t in enumerate(THRESHOLDS):
            y_true, y_score = [], []
            hits = {}                                             # (image, regular g) -> confidences of the predictions hitting it
            for k in per_class[c]:
                _, pixels, ignore, value, inter, size = (int(x) for x in rec[k, :6])
                conf = float(scores[k])
                if value >= 0 and float(inter) / (size + pixels - inter) > t:
                    if value >= 1000 and size >= min_region:
                        hits.setdefault((int(image[k]), value), []).append(conf)
                elif float(ignore) / pixels <= t:
                    y_true.append(0)
                    y_score.append(conf)
            for confs in hits.values():
                confs = sorted(confs)
                y_true.append(1)
                y_score.append(confs[-1])
                y_true.extend([0] * (len(confs) - 1))
                y_score.extend(confs[:-1])
            lists[(c, ti)] = (y_true, y_score, int(total_regular[c]) - len(hits))
    return lists, have_gt, have_pred


def _nanmean(values):
    have = [x for x in values if not x != x]
    return sum(have) / len(have) if have else float('nan')


def ap_from_records(rec, gt_regular, scores, image_offsets=None, min_region=MIN_REGION):
    """Everything after the records, in float64 on the host.  rec [N,8] and scores [N] of every prediction, gt_regular [M,8] of every
    image; image_offsets (None, one integer or [N]) is added to the records' image column, which counts within one call, to tell
    the images of different calls apart.  min_region must be the one the records were made with (it tells a hit on a regular region
    from a hit on a small one).  Returns {'ap' [8][10] (nan: the class has no regular ground truth), 'classes': {name: {'ap',
    'ap50%'}}, 'allAp', 'allAp50%'}."""
    lists, have_gt, have_pred = match_lists(rec, gt_regular, scores, image_offsets, min_region)
    ap = [[float('nan')] * len(THRESHOLDS) for _ in range(N_CLASSES)]
    for c in range(N_CLASSES):
        for ti in range(len(THRESHOLDS)):
            if have_gt[c] and have_pred[c]:
                ap[c][ti] = average_precision(*lists[(c, ti)])
            elif have_gt[c]:
                ap[c][ti] = 0.0
    return {'ap': ap,
            'classes': {CLASS_NAMES[c]: {'ap': _nanmean(ap[c]), 'ap50%': ap[c][0]} for c in range(N_CLASSES)},
            'allAp': _nanmean([x for row in ap for x in row]),
            'allAp50%': _nanmean([row[0] for row in ap])}


@torch.no_grad()
def masks_from_id_map(seg, fmt='trainid'):
    """A panoptic map -> (masks [P,H,W] u8, mask_image [P] int32, labels [P] int32 labelIds, scores [P] float64 = 1.0), one mask per
    thing segment in ascending value order image by image.  seg [B,H,W] or [H,W] integers, values label * 1000 + id for things
    with label a trainId ('trainid': what FGModel.predict_panoptic returns) or a labelId ('cityscapes': the decoded PNG of
    export_panoptic.py).  Plain torch on seg's device: not the hot path."""
    if fmt not in PANOPTIC_FORMATS:
        raise ValueError('fmt must be one of %s (got %r)' % (PANOPTIC_FORMATS, fmt))
    seg = torch.as_tensor(seg)
    if seg.dim() == 2:
        seg = seg[None]
    if seg.dim() != 3:
        raise ValueError('seg must be [B,H,W] or [H,W] (got %s)' % (tuple(seg.shape),))
    seg = seg.long()
    from .panoptic import TRAINID2ID
    masks, images, labels = [], [], []
    for i in range(seg.shape[0]):
        for v in torch.unique(seg[i][seg[i] >= 1000]).tolist():
            label = v // 1000
            if fmt == 'trainid':
                label = TRAINID2ID[label] if 0 <= label < len(TRAINID2ID) else -1
            if label not in INSTANCE_LABELS:
                continue
            masks.append((seg[i] == v).to(torch.uint8))
            images.append(i)
            labels.append(label)
    stack = torch.stack(masks) if masks else torch.zeros((0,) + tuple(seg.shape[1:]), dtype=torch.uint8, device=seg.device)
    return (stack, torch.tensor(images, dtype=torch.int32, device=seg.device), torch.tensor(labels, dtype=torch.int32, device=seg.device),
            torch.ones(len(masks), dtype=torch.float64, device=seg.device))


class InstanceAP(DeviceMeter):
    """Device-side instance-AP meter: ``update`` enqueues pf_ap_accumulate on the current stream and returns at once (no
    synchronisation, capturable); the records, region counts and float64 scores of every update stay on the device; ``result``
    waits, reads the status word and scores them with ap_from_records."""
    WORKSPACES = {'ap': ('_ws', '')}
    HOST_PATH = 'records_host'

    def __init__(self, min_region=MIN_REGION, device='cuda'):
        if min_region < 0:
            raise ValueError('min_region must not be negative')
        super().__init__(device)
        self.min_region = int(min_region)
        self._size = (0, 0)              # the largest (P, B) the workspace was sized for
        self._updates = []               # (rec [P,8], gt_regular [B,8] | None, scores [P] f64, image offset)
        self._images = 0

    def _workspace(self, dims, which):
        """DeviceMeter._workspace for a workspace of two dimensions: it grows with the largest (P, B) seen, each on its own, under
        the same capture rule."""
        p, b = max(dims[0], self._size[0]), max(dims[1], self._size[1])
        attr, label = self.WORKSPACES[which]
        old = getattr(self, attr)
        need = ctypes.c_size_t()
        self._call(which, 'workspace', p, b, ctypes.byref(need))
        capturing = torch.cuda.is_current_stream_capturing()
        if old is None or old.numel() < need.value:
            if capturing or self._captured:
                raise self._lib.PfError('%s: the %sworkspace would have to grow to (P, B) = (%d, %d) %s a graph capture, whose replays '
                                        'keep the old pointer: call %s() with the largest batch before capturing'
                                        % (type(self).__name__, label, p, b, 'during' if capturing else 'after', self.ENQUEUE))
            ws = torch.zeros(need.value, dtype=torch.uint8, device=self.device)    # status word starts at 0
            if old is not None:
                ws[:256].copy_(old[:256])                                            # a sticky bit survives the growth
            setattr(self, attr, ws)
        self._size = (p, b)
        self._captured = self._captured or capturing
        return getattr(self, attr)

    @torch.no_grad()
    def update(self, masks, mask_image, labels, scores, gt, new_images=True, out=None):
        """masks [P,H,W] u8 or bool (inside = non-zero), mask_image [P] int32 (index into gt; unsorted is fine), labels [P] int32
        labelIds, scores [P] confidences (kept as float64), gt [B,H,W] instance map (any 2-byte integer tensor is read as u16,
        i32 and i64 are taken as they are): device tensors, passed as they are.  new_images=False says that gt is the batch of the
        previous update again (an image's masks split over calls): its regions are not counted twice.  out: optional
        (rec [P,8] int32, gt_regular [B,8] int32) device tensors to write into (a captured update needs them: replays write there).
        Returns (rec, gt_regular)."""
        lib = self._lib
        L = lib.load()
        if masks.dtype == torch.bool:
            masks = masks.view(torch.uint8)
        if masks.dtype != torch.uint8 or masks.dim() != 3:
            raise lib.PfError('masks must be [P,H,W] u8 or bool (got %s %s)' % (masks.dtype, tuple(masks.shape)))
        if gt.dim() != 3 or tuple(gt.shape[1:]) != tuple(masks.shape[1:]):
            raise lib.PfError('gt must be [B,H,W] with the masks\' image shape (got %s and %s)' % (tuple(gt.shape), tuple(masks.shape)))
        integer = not (gt.dtype.is_floating_point or gt.dtype.is_complex or gt.dtype == torch.bool)
        if not integer or (gt.element_size() != 2 and gt.dtype not in _GT_KINDS):
            raise lib.PfError('gt must be a 16-bit, i32 or i64 integer instance map (got %s)' % gt.dtype)
        p, h, w = masks.shape
        b = gt.shape[0]
        for t, name in ((mask_image, 'mask_image'), (labels, 'labels')):
            if t.dtype != torch.int32 or tuple(t.shape) != (p,):
                raise lib.PfError('%s must be int32 [%d] (got %s %s)' % (name, p, t.dtype, tuple(t.shape)))
        if tuple(scores.shape) != (p,):
            raise lib.PfError('scores must be [%d] (got %s)' % (p, tuple(scores.shape)))
        for t, name in ((masks, 'masks'), (mask_image, 'mask_image'), (labels, 'labels'), (scores, 'scores'), (gt, 'gt')):
            lib.require_cuda(t, name)
        if h == 0 or w == 0:
            raise lib.PfError('masks and gt must hold pixels (got %s)' % (tuple(masks.shape),))
        if not new_images and (not self._updates or self._last_b != b):
            raise lib.PfError('new_images=False continues the previous update: it needs one, with a gt batch of the same size')
        if out is None:
            out = (torch.empty(p, 8, dtype=torch.int32, device=self.device), torch.empty(b, N_CLASSES, dtype=torch.int32, device=self.device))
        rec, regular = out
        for t, name, shape in ((rec, 'rec', (p, 8)), (regular, 'gt_regular', (b, N_CLASSES))):
            lib.require_cuda(t, 'out ' + name)
            if t.dtype != torch.int32 or tuple(t.shape) != shape:
                raise lib.PfError('out %s must be int32 %s' % (name, list(shape)))
        if p or b:
            ws = self._workspace((p, b), 'ap')
            lib.check(L.pf_ap_accumulate(masks.data_ptr(), mask_image.data_ptr(), labels.data_ptr(), p, gt.data_ptr(),
                                         _GT_KINDS.get(gt.dtype, 0), b, h, w, self.min_region, rec.data_ptr(), regular.data_ptr(),
                                         ws.data_ptr(), ws.numel(), lib.stream_ptr()), 'pf_ap_accumulate')
        offset = self._images if new_images else self._images - b
        self._updates.append((rec, regular if new_images else None, scores.to(torch.float64), offset))
        if new_images:
            self._images += b
        self._last_b = b
        return rec, regular

    def records(self):
        """(rec [N,8] int32 with the image column counting over all updates, gt_regular [M,8] int32, scores [N] float64) of every
        update so far, on the host (waits for the current stream)."""
        recs, regs, scores = [], [], []
        for rec, regular, s, offset in self._updates:
            r = rec.cpu().clone()
            ok = r[:, 0] != FLAGGED
            r[ok, 6] += offset
            recs.append(r)
            scores.append(s.cpu())
            if regular is not None:
                regs.append(regular.cpu())
        cat = lambda xs, shape, dt: torch.cat(xs) if xs else torch.zeros(shape, dtype=dt)
        return cat(recs, (0, 8), torch.int32), cat(regs, (0, N_CLASSES), torch.int32), cat(scores, (0,), torch.float64)

    def status(self):
        """The sticky status word (waits for the current stream)."""
        return self._status_word('ap')

    def result(self):
        """ap_from_records' dict over every update; PfError naming the bits when the status word is set."""
        st = self.status()
        if st:
            raise self._lib.PfError('instance AP status %d: %s (the flagged images and predictions add nothing; reset() clears this)'
                                    % (st, '; '.join(text for bit, text in STATUS_BITS if st & bit)))
        rec, regular, scores = self.records()
        return ap_from_records(rec, regular, scores, None, self.min_region)

    def reset(self):
        self._updates = []
        self._images = 0
        self._status_reset()
        return self
