"""Panoptic-quality accumulators for bg ("stuff") label maps + their cross-rank reduction.

The reference computes PQ with the external ``cityscapesscripts.evaluation.evalPanopticSemanticLabeling``
(scripts/fg/run_fg_eval_panoptic.sh:28-33; version unpinned, absent here => "parity unpinned").  This
restates the standard definition for stuff classes, where every class forms at most one segment per
image: a predicted and a ground-truth segment of the same class match iff IoU > 0.5 (void pixels,
label 255 in the ground truth, are removed from the prediction first);
    PQ_c = sum(IoU over TP) / (TP + FP/2 + FN/2),   PQ = mean over classes with TP+FP+FN > 0.
Accumulators are [n_cls, 4] float64 rows (sum_iou, TP, FP, FN): integer-valued counts add exactly, so a
sharded evaluation reproduces the single-process numbers (sum_iou to float64 rounding).
"""
import torch

from .meter import DeviceMeter

VOID = 255


def pq_accumulate(pred, gt, n_cls, acc=None):
    """pred, gt: [B,H,W] integer label maps (any device). Returns/updates acc [n_cls,4] float64 on that device."""
    if acc is None:
        acc = torch.zeros(n_cls, 4, dtype=torch.float64, device=pred.device)
    b = pred.shape[0]
    p = pred.reshape(b, -1).long()
    g = gt.reshape(b, -1).long()
    keep = g != VOID
    pc = torch.where(keep & (p < n_cls), p, torch.full_like(p, n_cls))      # bucket n_cls = ignored
    gc = torch.where(keep & (g < n_cls), g, torch.full_like(g, n_cls))
    k = n_cls + 1
    idx = (torch.arange(b, device=p.device).view(b, 1) * k + gc) * k + pc
    conf = torch.bincount(idx.reshape(-1), minlength=b * k * k).view(b, k, k)[:, :n_cls + 1, :n_cls + 1].double()
    inter = torch.diagonal(conf, dim1=1, dim2=2)[:, :n_cls]                  # [B, n_cls]
    g_area = conf.sum(2)[:, :n_cls]
    p_area = conf[:, :n_cls + 1, :n_cls].sum(1)                               # predictions on non-void gt pixels
    union = g_area + p_area - inter
    iou = torch.where(union > 0, inter / union.clamp(min=1), torch.zeros_like(union))
    tp = iou > 0.5
    fp = (p_area > 0) & ~tp
    fn = (g_area > 0) & ~tp
    acc[:, 0] += (iou * tp).sum(0)
    acc[:, 1] += tp.sum(0).double()
    acc[:, 2] += fp.sum(0).double()
    acc[:, 3] += fn.sum(0).double()
    return acc


def pq_from_acc(acc):
    """{'pq','sq','rq','per_class'} in percent from [n_cls,4] accumulators."""
    acc = acc.double().cpu()
    siou, tp, fp, fn = acc[:, 0], acc[:, 1], acc[:, 2], acc[:, 3]
    denom = tp + 0.5 * fp + 0.5 * fn
    have = denom > 0
    pq_c = torch.where(have, siou / denom.clamp(min=1e-12), torch.zeros_like(siou))
    sq_c = torch.where(tp > 0, siou / tp.clamp(min=1), torch.zeros_like(siou))
    rq_c = torch.where(have, tp / denom.clamp(min=1e-12), torch.zeros_like(siou))
    n = max(int(have.sum()), 1)
    return {'pq': 100.0 * float(pq_c[have].sum()) / n, 'sq': 100.0 * float(sq_c[have].sum()) / n,
            'rq': 100.0 * float(rq_c[have].sum()) / n, 'per_class': (100.0 * pq_c).tolist(),
            'n_classes': int(have.sum())}


def _category(ids):
    return torch.where(ids > 100, ids // 1000, ids)


def pq_accumulate_panoptic(pred, gt, n_cls=19, acc=None):
    """Panoptic maps with instances: [B,H,W] integer maps in the merge output format (stuff = trainId, thing =
    (trainId)*1000 + instance, void = 255; panoptic.py / fg_model.py:572).  Standard PQ matching: a predicted and a
    ground-truth segment of the same category match iff IoU > 0.5, the union not counting predicted pixels on void;
    unmatched predictions lying more than half on void are not false positives.  Same [n_cls,4] accumulators as
    pq_accumulate (the segment tables are tiny: the matching itself runs on the host)."""
    if acc is None:
        acc = torch.zeros(n_cls, 4, dtype=torch.float64, device=pred.device)
    add = torch.zeros(n_cls, 4, dtype=torch.float64)
    for b in range(pred.shape[0]):
        p = pred[b].reshape(-1).long()
        g = gt[b].reshape(-1).long()
        uk, cnt = torch.unique(g * 65536 + p, return_counts=True)
        uk, cnt = uk.cpu(), cnt.cpu().double()
        ug, up = uk // 65536, uk % 65536
        g_ids, g_inv = torch.unique(ug, return_inverse=True)
        p_ids, p_inv = torch.unique(up, return_inverse=True)
        g_area = torch.zeros(len(g_ids), dtype=torch.float64).index_add_(0, g_inv, cnt)
        p_area = torch.zeros(len(p_ids), dtype=torch.float64).index_add_(0, p_inv, cnt)
        p_void = torch.zeros(len(p_ids), dtype=torch.float64).index_add_(0, p_inv, cnt * (ug == VOID))
        g_cat, p_cat = _category(g_ids), _category(p_ids)
        g_hit = torch.zeros(len(g_ids), dtype=torch.bool)
        p_hit = torch.zeros(len(p_ids), dtype=torch.bool)
        same = (g_cat[g_inv] == p_cat[p_inv]) & (ug != VOID) & (up != VOID) & (g_cat[g_inv] < n_cls)
        union = g_area[g_inv] + p_area[p_inv] - cnt - p_void[p_inv]
        iou = cnt / union.clamp(min=1)
        for k in torch.nonzero(same & (iou > 0.5)).flatten().tolist():
            c = int(g_cat[g_inv[k]])
            add[c, 0] += float(iou[k])
            add[c, 1] += 1
            g_hit[g_inv[k]] = True
            p_hit[p_inv[k]] = True
        for i in range(len(g_ids)):
            if not g_hit[i] and g_ids[i] != VOID and g_cat[i] < n_cls:
                add[int(g_cat[i]), 3] += 1
        for i in range(len(p_ids)):
            if not p_hit[i] and p_ids[i] != VOID and p_cat[i] < n_cls and p_void[i] <= 0.5 * p_area[i]:
                add[int(p_cat[i]), 2] += 1
    acc += add.to(acc.device)
    return acc


# ---------------------------------------------------------------------------------------------------------------------
# Panoptic quality with void, crowd and both id formats: the semantics of include/pfhip.h's pf_pq_accumulate block.
# pq_panoptic_host states them in torch + host code (any device; the CPU path of eval_panoptic.py); PanopticQuality
# enqueues the HIP kernels (csrc/pq_kernels.hip).  tests/pq_ref64.py restates them a third time, without either.

FORMATS = {'trainid': 0, 'cityscapes': 1}
FIRST_THING = 11                       # trainIds 11..18 are the thing classes
STATUS_BITS = ((1, 'PF_PQ_STATUS_FULL: an image holds more distinct (gt, pred) pairs than the table has slots'),
               (2, 'PF_PQ_STATUS_VALUE: a label value outside [0, 65536)'))
_VOID_ID = 65536                       # pseudo-segment of everything void


def _trainid_lut(fmt, n_cls):
    """value base (v // 1000 for v >= 1000, else v; below 1000 either way) -> trainId, -1 = void."""
    if fmt not in FORMATS:
        raise ValueError('fmt must be one of %s (got %r)' % (sorted(FORMATS), fmt))
    lut = torch.full((1000,), -1, dtype=torch.int64)
    if fmt == 'trainid':
        lut[:n_cls] = torch.arange(n_cls)
    else:
        from .panoptic import TRAINID2ID
        for t, i in enumerate(TRAINID2ID[:n_cls]):
            lut[i] = t
    return lut


def _base(ids):
    return torch.where(ids >= 1000, ids // 1000, ids)


def pq_panoptic_host(pred, gt, n_cls=19, fmt='trainid', crowd=True, acc=None):
    """pred, gt: [B,H,W] integer maps (any device) in ``fmt`` ('trainid': the merge output, void 255; 'cityscapes': decoded
    PNG ids, void 0).  A pixel is void when its category is none of the n_cls classes; with ``crowd`` a ground-truth segment
    without instance part (v < 1000) of a thing class is crowd: never TP or FN, and it excuses unmatched predictions of its
    own category lying more than half on void + crowd.  Returns/updates acc [n_cls,4] float64 (sum_iou, TP, FP, FN): the
    ious of a class are added in ascending gt id per image, the images in order."""
    if not 1 <= n_cls <= 19:
        raise ValueError('n_cls must be 1..19')
    if acc is None:
        acc = torch.zeros(n_cls, 4, dtype=torch.float64, device=pred.device)
    lut = _trainid_lut(fmt, n_cls)
    for b in range(pred.shape[0]):
        p = pred[b].reshape(-1).long()
        g = gt[b].reshape(-1).long()
        if p.numel() and (int(torch.minimum(p.min(), g.min())) < 0 or int(torch.maximum(p.max(), g.max())) > 65535):
            raise ValueError('image %d: label value outside [0, 65536)' % b)
        uk, cnt = torch.unique(g * 65536 + p, return_counts=True)          # sorted: ascending gt id, then pred id
        uk, cnt = uk.cpu(), cnt.cpu()
        ug, up = uk // 65536, uk % 65536
        gc, pc = lut[_base(ug)], lut[_base(up)]
        g_void, p_void_px = gc < 0, pc < 0
        g_crowd = (ug < 1000) & (gc >= FIRST_THING) if crowd else torch.zeros_like(g_void)
        g_ids, g_inv = torch.unique(torch.where(g_void, torch.full_like(ug, _VOID_ID), ug), return_inverse=True)
        p_ids, p_inv = torch.unique(torch.where(p_void_px, torch.full_like(up, _VOID_ID), up), return_inverse=True)
        g_area = torch.zeros(len(g_ids), dtype=torch.int64).index_add_(0, g_inv, cnt)
        p_area = torch.zeros(len(p_ids), dtype=torch.int64).index_add_(0, p_inv, cnt)
        p_on_void = torch.zeros(len(p_ids), dtype=torch.int64).index_add_(0, p_inv, cnt * g_void)
        p_on_crowd = torch.zeros(len(p_ids), dtype=torch.int64).index_add_(0, p_inv, cnt * (g_crowd & (gc == pc)))
        union = g_area[g_inv] + p_area[p_inv] - cnt - p_on_void[p_inv]
        iou = cnt.double() / union.clamp(min=1).double()
        tp = ~g_void & ~g_crowd & (gc == pc) & (iou > 0.5)
        add = torch.zeros(n_cls, 4, dtype=torch.float64)
        g_hit = torch.zeros(len(g_ids), dtype=torch.bool)
        p_hit = torch.zeros(len(p_ids), dtype=torch.bool)
        for k in torch.nonzero(tp).flatten().tolist():
            add[int(gc[k]), 0] += float(iou[k])
            add[int(gc[k]), 1] += 1
            g_hit[g_inv[k]] = True
            p_hit[p_inv[k]] = True
        g_cat = torch.full((len(g_ids),), -1, dtype=torch.int64).index_put_((g_inv,), gc)
        g_is_crowd = torch.zeros(len(g_ids), dtype=torch.bool).index_put_((g_inv,), g_crowd)
        p_cat = torch.full((len(p_ids),), -1, dtype=torch.int64).index_put_((p_inv,), pc)
        for i in torch.nonzero((g_cat >= 0) & ~g_is_crowd & ~g_hit).flatten().tolist():
            add[int(g_cat[i]), 3] += 1
        fp = (p_cat >= 0) & ~p_hit & ~(2 * (p_on_void + p_on_crowd) > p_area)
        for i in torch.nonzero(fp).flatten().tolist():
            add[int(p_cat[i]), 2] += 1
        acc += add.to(acc.device)
    return acc


def pq_splits(acc, scale=100.0):
    """{'All','Things','Stuff'}: {'pq','sq','rq','n'} (means over the classes with TP+FP+FN > 0, times ``scale``) and
    'per_class': [{'pq','sq','rq'}] from [n_cls,4] accumulators; things are trainIds 11..18."""
    acc = acc.double().cpu()
    siou, tp, fp, fn = acc[:, 0], acc[:, 1], acc[:, 2], acc[:, 3]
    denom = tp + 0.5 * fp + 0.5 * fn
    have = denom > 0
    pq_c = torch.where(have, siou / denom.clamp(min=1e-12), torch.zeros_like(siou))
    sq_c = torch.where(tp > 0, siou / tp.clamp(min=1), torch.zeros_like(siou))
    rq_c = torch.where(have, tp / denom.clamp(min=1e-12), torch.zeros_like(siou))
    thing = torch.arange(acc.shape[0]) >= FIRST_THING
    out = {}
    for name, sel in (('All', have), ('Things', have & thing), ('Stuff', have & ~thing)):
        n = int(sel.sum())
        d = max(n, 1)
        out[name] = {'pq': scale * float(pq_c[sel].sum()) / d, 'sq': scale * float(sq_c[sel].sum()) / d,
                     'rq': scale * float(rq_c[sel].sum()) / d, 'n': n}
    out['per_class'] = [{'pq': scale * float(pq_c[c]), 'sq': scale * float(sq_c[c]), 'rq': scale * float(rq_c[c])}
                        for c in range(acc.shape[0])]
    return out


class PanopticQuality(DeviceMeter):
    """Device-side panoptic quality: ``update`` enqueues pf_pq_accumulate on the current stream and returns at once (no
    synchronisation, capturable), ``acc`` is the [n_cls,4] float64 device tensor, ``result`` waits and reads the status word."""
    WORKSPACES = {'pq': ('_ws', '')}
    HOST_PATH = 'pq_panoptic_host'

    def __init__(self, n_cls=19, fmt='trainid', crowd=True, device='cuda'):
        if fmt not in FORMATS:
            raise ValueError('fmt must be one of %s (got %r)' % (sorted(FORMATS), fmt))
        if not 1 <= n_cls <= 19:
            raise ValueError('n_cls must be 1..19')
        super().__init__(device)
        self.n_cls, self.fmt, self.crowd = n_cls, fmt, bool(crowd)
        self.acc = torch.zeros(n_cls, 4, dtype=torch.float64, device=self.device)

    @torch.no_grad()
    def update(self, pred, gt, per_image=None):
        """pred, gt [B,H,W] i32 or i64 (u8, i8 and i16 are widened to i32 on the device; any other dtype is refused);
        per_image: optional [B,n_cls,4] float64 device tensor that receives each image's row."""
        L, lib = self._lib.load(), self._lib
        if pred.dim() != 3 or pred.shape != gt.shape:
            raise lib.PfError('pred and gt must be [B,H,W] of one shape (got %s and %s)' % (tuple(pred.shape), tuple(gt.shape)))
        maps = []
        for t, name in ((pred, 'pred'), (gt, 'gt')):
            lib.require_cuda(t, name)
            if t.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
                raise lib.PfError('%s must be an integer label map (got %s)' % (name, t.dtype))
            maps.append(t if t.dtype in (torch.int32, torch.int64) else t.to(torch.int32))
        b, h, w = pred.shape
        if b == 0:
            return self
        if per_image is not None:
            lib.require_cuda(per_image, 'per_image')
            if per_image.dtype != torch.float64 or tuple(per_image.shape) != (b, self.n_cls, 4):
                raise lib.PfError('per_image must be float64 [%d,%d,4]' % (b, self.n_cls))
        ws = self._workspace(b, 'pq')
        lib.check(L.pf_pq_accumulate(maps[0].data_ptr(), int(maps[0].dtype == torch.int64), maps[1].data_ptr(),
                                     int(maps[1].dtype == torch.int64), FORMATS[self.fmt], int(self.crowd), self.n_cls, b, h, w,
                                     self.acc.data_ptr(), per_image.data_ptr() if per_image is not None else None,
                                     ws.data_ptr(), ws.numel(), lib.stream_ptr()), 'pf_pq_accumulate')
        return self

    def status(self):
        """The sticky status word (waits for the current stream)."""
        return self._status_word('pq')

    def result(self):
        """pq_from_acc's dict plus the 'All' / 'Things' / 'Stuff' split; PfError naming the bit when the status word is set."""
        st = self.status()
        if st:
            raise self._lib.PfError('panoptic quality status %d: %s (the flagged images were left out of acc; reset() clears this)'
                                    % (st, '; '.join(text for bit, text in STATUS_BITS if st & bit)))
        out = pq_from_acc(self.acc)
        split = pq_splits(self.acc)
        out.update({k: split[k] for k in ('All', 'Things', 'Stuff')})
        return out

    def reset(self):
        self.acc.zero_()
        self._status_reset()
        return self
