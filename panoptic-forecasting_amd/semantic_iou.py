"""Semantic confusion matrix, IoU and mIoU for label maps: the semantics of include/pfhip.h's pf_confusion_accumulate block.

The reference leaves the scoring of its semantic outputs (the bg forecast of ``export_bg.py``, ``FGModel.predict_semantics``) to the
external ``cityscapesscripts.evaluation.evalPixelLevelSemanticLabeling``; that package is absent here and its version unpinned, so
the formula below is written down from the Cityscapes pixel-level evaluator as remembered: parity unpinned.
iIoU (instance-weighted) and the seven category scores are built the same way, from the evaluator's definition and class-size table
as remembered (pf_iiou_accumulate block): parity unpinned too.

``confusion_host`` / ``instance_sums_host`` state the counting in torch (any device; the host path of eval_semantic.py);
``SemanticIoU`` enqueues the HIP kernels (csrc/confusion_kernels.hip, csrc/iiou_kernels.hip); tests/conf_ref64.py and
tests/iiou_ref64.py restate both a third time, without either.

A confusion table is [20,20] int64: row = ground-truth class, column = predicted class, index 19 = void.  Integers add exactly, so
a sharded evaluation reproduces the single-process table bit for bit.

The instance sums are float64 and their order is fixed: per image and thing class the terms of its instances are added in
ascending instance value from 0.0 into (itp, ifn); a meter adds the images' pairs in update order.  An image's pairs are the unit of
exchange: they are bit-identical whatever batch the image is in, and a sharded evaluation adds them in one global order.
"""
import torch

from .meter import DeviceMeter

FORMATS = {'trainid': 0, 'cityscapes': 1}
N_CELLS = 20                           # 19 classes + void
VOID = 19
FIRST_MO = 11                          # trainIds 0..10 are stuff, 11..18 the moving objects
STATUS_BITS = ((1, 'PF_CONF_STATUS_VALUE: a label value outside [0, 256)'),)
_KINDS = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}
N_THINGS = 8                           # trainIds 11..18
IIOU_STATUS_BITS = ((1, 'PF_IIOU_STATUS_VALUE: a prediction value outside [0, 256) or an instance value outside [0, 65536)'),)
_INST_KINDS = {torch.int32: 1, torch.int64: 2}           # any 2-byte integer tensor is read as u16: kind 0
# the evaluator's average instance size per thing class, as remembered (csrc/iiou_kernels.hip: kIiouAvgSize is the device's copy)
AVG_CLASS_SIZE = (3462.4756337644, 3930.4788056518, 12794.0202738185, 27855.1264367816, 35732.1511111111, 67422.8757396450,
                  6298.7200839748, 4672.3249222261)
CATEGORIES = (('flat', (0, 1)), ('construction', (2, 3, 4)), ('object', (5, 6, 7)), ('nature', (8, 9)), ('sky', (10,)),
              ('human', (11, 12)), ('vehicle', (13, 14, 15, 16, 17, 18)))


def class_lut(fmt, n_cls):
    """value 0..255 -> class 0..n_cls-1, 19 = void."""
    if fmt not in FORMATS:
        raise ValueError('fmt must be one of %s (got %r)' % (sorted(FORMATS), fmt))
    if not 1 <= n_cls <= 19:
        raise ValueError('n_cls must be 1..19')
    lut = torch.full((256,), VOID, dtype=torch.int64)
    if fmt == 'trainid':
        lut[:n_cls] = torch.arange(n_cls)
    else:
        from .panoptic import TRAINID2ID
        for t, i in enumerate(TRAINID2ID[:n_cls]):
            lut[i] = t
    return lut


def confusion_host(pred, gt, n_cls=19, fmt='trainid', acc=None):
    """pred, gt: integer label maps of one shape (any device) in ``fmt`` ('trainid': 0..18 are classes, everything else void;
    'cityscapes': labelIds, every id without a trainId void).  A value whose class is >= n_cls is void.  Returns/updates acc [20,20]
    int64 (row = gt class, column = predicted class, 19 = void) on the maps' device.  A value outside [0, 256): ValueError."""
    lut = class_lut(fmt, n_cls).to(pred.device)
    if pred.shape != gt.shape:
        raise ValueError('pred and gt must have one shape (got %s and %s)' % (tuple(pred.shape), tuple(gt.shape)))
    if acc is None:
        acc = torch.zeros(N_CELLS, N_CELLS, dtype=torch.int64, device=pred.device)
    p, g = pred.reshape(-1).long(), gt.reshape(-1).long()
    if p.numel() == 0:
        return acc
    if int(torch.minimum(p.min(), g.min())) < 0 or int(torch.maximum(p.max(), g.max())) > 255:
        raise ValueError('label value outside [0, 256)')
    acc += torch.bincount(lut[g] * N_CELLS + lut[p], minlength=N_CELLS * N_CELLS).view(N_CELLS, N_CELLS).to(acc.device)
    return acc


def iou_from_confusion(acc, scale=100.0):
    """{'All','Stuff','MO'}: {'miou','n'} (means over the classes present, times ``scale``), 'per_class' (``scale`` x iou, nan for an
    absent class) and 'pixel_acc' (``scale`` x trace / pixels of non-void ground truth) from a [20,20] table.  Per class c:
    tp = acc[c,c]; fn = acc[c,:].sum() - tp (the void column included: a void prediction on valid ground truth is a miss);
    fp = acc[:19,c].sum() - tp (the void row excluded: ignored ground truth excuses the prediction); iou = tp / (tp + fp + fn),
    one fp64 division of integers.  A class with tp + fp + fn == 0 is absent: left out of the means."""
    acc = torch.as_tensor(acc).cpu().to(torch.int64)
    if tuple(acc.shape) != (N_CELLS, N_CELLS):
        raise ValueError('acc must be [20,20] (got %s)' % (tuple(acc.shape),))
    tp = torch.diagonal(acc)[:VOID]
    fn = acc[:VOID, :].sum(1) - tp
    fp = acc[:VOID, :VOID].sum(0) - tp
    denom = tp + fp + fn
    have = denom > 0
    iou = torch.where(have, tp.double() / denom.clamp(min=1).double(), torch.full((VOID,), float('nan'), dtype=torch.float64))
    mo = torch.arange(VOID) >= FIRST_MO
    out = {}
    for name, sel in (('All', have), ('Stuff', have & ~mo), ('MO', have & mo)):
        n = int(sel.sum())
        out[name] = {'miou': scale * float(iou[sel].sum()) / n if n else float('nan'), 'n': n}
    out['per_class'] = [scale * float(x) for x in iou]
    valid = int(acc[:VOID, :].sum())
    out['pixel_acc'] = scale * float(tp.sum().double() / valid) if valid else float('nan')
    return out


def _instance_values(inst):
    """Instance map -> int64 values; a 2-byte integer tensor is read as u16 (as hop_io reads depth codes)."""
    inst = torch.as_tensor(inst)
    if inst.dtype.is_floating_point or inst.dtype.is_complex or inst.dtype == torch.bool:
        raise ValueError('inst must be an integer instance map (got %s)' % inst.dtype)
    if inst.element_size() == 2:
        return inst.view(torch.int16).long() & 0xffff
    return inst.long()


def instance_sums_host(pred, inst, n_cls=19, fmt='trainid'):
    """pred [B,H,W] label map in ``fmt``, inst [B,H,W] ground-truth instance map (always labelIds: labelId * 1000 + k), any
    device.  Returns (per_image [B,8,2] float64 (itp, ifn), per_image_counts [B,8,3] int64 (instances, pixels, tp pixels)) on the
    host, per thing class 11..18: the pf_iiou_accumulate block of include/pfhip.h stated with ``torch.unique``.  Per image, the
    distinct values v > 1000 in ascending order; label v // 1000 -> trainId c; 11 <= c < n_cls counts, everything else is ignored.
    w = avg[c] / size, itp += tp * w, ifn += (size - tp) * w in Python floats (float64, one rounding each, from 0.0).
    A prediction value outside [0, 256) or an instance value outside [0, 65536): ValueError."""
    if fmt not in FORMATS:
        raise ValueError('fmt must be one of %s (got %r)' % (sorted(FORMATS), fmt))
    if not 1 <= n_cls <= 19:
        raise ValueError('n_cls must be 1..19')
    pred = torch.as_tensor(pred)
    v = _instance_values(inst)
    if pred.dim() != 3 or pred.shape != v.shape:
        raise ValueError('pred and inst must be [B,H,W] of one shape (got %s and %s)' % (tuple(pred.shape), tuple(v.shape)))
    from .panoptic import TRAINID2ID
    b = pred.shape[0]
    sums = [[[0.0, 0.0] for _ in range(N_THINGS)] for _ in range(b)]
    counts = [[[0, 0, 0] for _ in range(N_THINGS)] for _ in range(b)]
    if pred.numel():
        p, v = pred.reshape(b, -1).long(), v.reshape(b, -1).to(pred.device)
        if int(p.min()) < 0 or int(p.max()) > 255 or int(v.min()) < 0 or int(v.max()) > 65535:
            raise ValueError('prediction value outside [0, 256) or instance value outside [0, 65536)')
        thing_of_label = torch.full((66,), -1, dtype=torch.int64)
        for t in range(N_THINGS):
            if FIRST_MO + t < n_cls:
                thing_of_label[TRAINID2ID[FIRST_MO + t]] = t
        thing_of_label = thing_of_label.to(p.device)
        for i in range(b):
            sel = v[i] > 1000
            uv, inverse, size = torch.unique(v[i][sel], sorted=True, return_inverse=True, return_counts=True)
            if uv.numel() == 0:
                continue
            label = uv // 1000
            thing = thing_of_label[label]
            want = label if fmt == 'cityscapes' else thing + FIRST_MO
            tp = torch.bincount(inverse[p[i][sel] == want[inverse]], minlength=uv.numel())
            for t, n, hit in zip(thing.tolist(), size.tolist(), tp.tolist()):          # ascending v
                if t < 0:
                    continue
                w = AVG_CLASS_SIZE[t] / float(n)
                sums[i][t][0] += float(hit) * w
                sums[i][t][1] += float(n - hit) * w
                counts[i][t][0] += 1
                counts[i][t][1] += n
                counts[i][t][2] += hit
    return (torch.tensor(sums, dtype=torch.float64).reshape(b, N_THINGS, 2),
            torch.tensor(counts, dtype=torch.int64).reshape(b, N_THINGS, 3))


def _table(acc):
    acc = torch.as_tensor(acc).cpu().to(torch.int64)
    if tuple(acc.shape) != (N_CELLS, N_CELLS):
        raise ValueError('acc must be [20,20] (got %s)' % (tuple(acc.shape),))
    return acc.tolist()


def _pairs(acc_inst):
    s = torch.as_tensor(acc_inst).cpu().to(torch.float64)
    if tuple(s.shape) != (N_THINGS, 2):
        raise ValueError('acc_inst must be [8,2] (got %s)' % (tuple(s.shape),))
    return s.tolist()


def _mean(values, scale):
    have = [x for x in values if not x != x]
    return {'miou': scale * sum(have) / len(have) if have else float('nan'), 'n': len(have)}


def iiou_from_sums(acc, acc_inst, scale=100.0):
    """{'miou','n','per_class'} of the eight thing classes 11..18 from the [20,20] table and the [8,2] (itp, ifn) sums:
    iIoU = itp / (itp + fp + ifn) with fp = acc[:19,c].sum() - acc[c,c], the unweighted false positives of iou_from_confusion;
    nan where the denominator is 0, the mean over the classes present; times ``scale``."""
    t, s = _table(acc), _pairs(acc_inst)
    per = []
    for k in range(N_THINGS):
        c = FIRST_MO + k
        fp = sum(t[g][c] for g in range(VOID)) - t[c][c]
        d = s[k][0] + float(fp) + s[k][1]
        per.append(s[k][0] / d if d > 0 else float('nan'))
    out = _mean(per, scale)
    out['per_class'] = [scale * x for x in per]
    return out


def category_scores(acc, acc_inst=None, scale=100.0):
    """The seven Cityscapes categories (CATEGORIES: sets S of trainIds) from the [20,20] table: tp = acc[S][:,S].sum(),
    fn = acc[S,:].sum() - tp (void column included), fp = acc[rows 0..18 outside S][:,S].sum(); iou = tp / (tp + fp + fn).
    With acc_inst, human and vehicle also get iiou = itp / (itp + fp + ifn) from their classes' sums added in class order.
    Returns {'per_category': {name: {'iou', 'iiou'}}, 'iou': {'miou','n'}, 'iiou': {'miou','n'}}: nan = absent, means over the
    categories present, times ``scale``."""
    t = _table(acc)
    s = _pairs(acc_inst) if acc_inst is not None else None
    nan = float('nan')
    per = {}
    for name, members in CATEGORIES:
        tp = sum(t[g][p] for g in members for p in members)
        fn = sum(t[g][p] for g in members for p in range(N_CELLS)) - tp
        fp = sum(t[g][p] for g in range(VOID) if g not in members for p in members)
        d = tp + fp + fn
        iiou = nan
        if s is not None and members[0] >= FIRST_MO:
            itp = ifn = 0.0
            for c in members:
                itp += s[c - FIRST_MO][0]
                ifn += s[c - FIRST_MO][1]
            di = itp + float(fp) + ifn
            iiou = itp / di if di > 0 else nan
        per[name] = {'iou': tp / d if d else nan, 'iiou': iiou}
    out = {'iou': _mean([x['iou'] for x in per.values()], scale), 'iiou': _mean([x['iiou'] for x in per.values()], scale)}
    out['per_category'] = {name: {k: scale * x for k, x in v.items()} for name, v in per.items()}
    return out


class SemanticIoU(DeviceMeter):
    """Device-side confusion meter: ``update`` enqueues pf_confusion_accumulate (and, given an instance map, pf_iiou_accumulate)
    on the current stream and returns at once (no synchronisation, capturable), ``acc`` is the [20,20] int64 device tensor,
    ``acc_inst`` / ``acc_inst_counts`` the [8,2] float64 / [8,3] int64 instance sums, ``result`` waits and reads the status words."""
    WORKSPACES = {'confusion': ('_ws', 'confusion '), 'iiou': ('_ws_inst', 'iiou ')}   # the iIoU calls have a workspace and a status word of their own
    HOST_PATH = 'confusion_host'

    def __init__(self, n_cls=19, fmt='trainid', device='cuda'):
        if fmt not in FORMATS:
            raise ValueError('fmt must be one of %s (got %r)' % (sorted(FORMATS), fmt))
        if not 1 <= n_cls <= 19:
            raise ValueError('n_cls must be 1..19')
        super().__init__(device)
        self.n_cls, self.fmt = n_cls, fmt
        self.acc = torch.zeros(N_CELLS, N_CELLS, dtype=torch.int64, device=self.device)
        self.acc_inst = torch.zeros(N_THINGS, 2, dtype=torch.float64, device=self.device)
        self.acc_inst_counts = torch.zeros(N_THINGS, 3, dtype=torch.int64, device=self.device)
        self._updates = [0, 0]           # updates without / with an instance map

    @torch.no_grad()
    def update(self, pred, gt, per_image=None, inst=None, per_image_inst=None, per_image_inst_counts=None):
        """pred, gt [B,H,W] u8, i32 or i64, passed as they are, each in its own width (i8 and i16 are widened to i32 on the device;
        any other dtype is refused); per_image: optional [B,20,20] int64 device tensor that receives each image's table.
        inst: optional [B,H,W] ground-truth instance map (labelId * 1000 + k): any 2-byte integer tensor is read as u16, i32 and
        i64 are taken as they are, anything else is refused.  With it pf_iiou_accumulate is enqueued after the confusion call and
        adds to acc_inst / acc_inst_counts; per_image_inst [B,8,2] float64 and per_image_inst_counts [B,8,3] int64 (optional
        device tensors) receive each image's blocks."""
        L, lib = self._lib.load(), self._lib
        if inst is None and (per_image_inst is not None or per_image_inst_counts is not None):
            raise lib.PfError('per_image_inst / per_image_inst_counts need inst')
        if pred.dim() != 3 or pred.shape != gt.shape:
            raise lib.PfError('pred and gt must be [B,H,W] of one shape (got %s and %s)' % (tuple(pred.shape), tuple(gt.shape)))
        maps = []
        for t, name in ((pred, 'pred'), (gt, 'gt')):
            lib.require_cuda(t, name)
            if t.dtype not in _KINDS and t.dtype not in (torch.int8, torch.int16):
                raise lib.PfError('%s must be an integer label map (got %s)' % (name, t.dtype))
            maps.append(t if t.dtype in _KINDS else t.to(torch.int32))
        if inst is not None:
            if inst.shape != pred.shape:
                raise lib.PfError('inst must have the shape of pred (got %s and %s)' % (tuple(inst.shape), tuple(pred.shape)))
            lib.require_cuda(inst, 'inst')
            integer = not (inst.dtype.is_floating_point or inst.dtype.is_complex or inst.dtype == torch.bool)
            if not integer or (inst.element_size() != 2 and inst.dtype not in _INST_KINDS):
                raise lib.PfError('inst must be a 16-bit, i32 or i64 integer instance map (got %s)' % inst.dtype)
        b, h, w = pred.shape
        if b == 0:
            return self
        if h == 0 or w == 0:
            raise lib.PfError('pred and gt must hold pixels (got %s)' % (tuple(pred.shape),))
        if per_image is not None:
            lib.require_cuda(per_image, 'per_image')
            if per_image.dtype != torch.int64 or tuple(per_image.shape) != (b, N_CELLS, N_CELLS):
                raise lib.PfError('per_image must be int64 [%d,%d,%d]' % (b, N_CELLS, N_CELLS))
        for t, name, dtype, last in ((per_image_inst, 'per_image_inst', torch.float64, 2),
                                     (per_image_inst_counts, 'per_image_inst_counts', torch.int64, 3)):
            if t is not None:
                lib.require_cuda(t, name)
                if t.dtype != dtype or tuple(t.shape) != (b, N_THINGS, last):
                    raise lib.PfError('%s must be %s [%d,%d,%d]' % (name, str(dtype).split('.')[1], b, N_THINGS, last))
        ws = self._workspace(b, 'confusion')
        ws_inst = self._workspace(b, 'iiou') if inst is not None else None     # both sized before anything is enqueued
        lib.check(L.pf_confusion_accumulate(maps[0].data_ptr(), _KINDS[maps[0].dtype], maps[1].data_ptr(), _KINDS[maps[1].dtype],
                                            FORMATS[self.fmt], self.n_cls, b, h, w, self.acc.data_ptr(),
                                            per_image.data_ptr() if per_image is not None else None,
                                            ws.data_ptr(), ws.numel(), lib.stream_ptr()), 'pf_confusion_accumulate')
        self._updates[inst is not None] += 1
        if inst is not None:
            ptr = lambda t: t.data_ptr() if t is not None else None
            lib.check(L.pf_iiou_accumulate(maps[0].data_ptr(), _KINDS[maps[0].dtype], inst.data_ptr(), _INST_KINDS.get(inst.dtype, 0),
                                           FORMATS[self.fmt], self.n_cls, b, h, w, self.acc_inst.data_ptr(),
                                           self.acc_inst_counts.data_ptr(), ptr(per_image_inst), ptr(per_image_inst_counts),
                                           ws_inst.data_ptr(), ws_inst.numel(), lib.stream_ptr()), 'pf_iiou_accumulate')
        return self

    def _status_words(self):
        """(confusion status word, iIoU status word); waits for the current stream."""
        return self._status_word('confusion'), self._status_word('iiou')

    def status(self):
        """The sticky status words ORed (both calls use bit 1 for a value out of range; waits for the current stream)."""
        conf, inst = self._status_words()
        return conf | inst

    def result(self):
        """iou_from_confusion's dict; after updates with an instance map also 'iIoU' (iiou_from_sums) and 'categories'
        (category_scores).  PfError naming the bit when a status word is set, and when the meter has seen updates both with and
        without an instance map (its false positives would count images its instance sums do not)."""
        conf, inst = self._status_words()
        if conf or inst:
            texts = [text for bit, text in STATUS_BITS if conf & bit] + [text for bit, text in IIOU_STATUS_BITS if inst & bit]
            raise self._lib.PfError('semantic IoU status %d: %s (the flagged images were left out of acc; reset() clears this)'
                                    % (conf | inst, '; '.join(texts)))
        without, with_inst = self._updates
        if without and with_inst:
            raise self._lib.PfError('SemanticIoU: %d updates came with an instance map and %d without: iIoU needs the false positives '
                                    'of exactly the images whose instances were summed (reset() clears this)' % (with_inst, without))
        out = iou_from_confusion(self.acc)
        if with_inst:
            out['iIoU'] = iiou_from_sums(self.acc, self.acc_inst)
            out['categories'] = category_scores(self.acc, self.acc_inst)
        return out

    def reset(self):
        self.acc.zero_()
        self.acc_inst.zero_()
        self.acc_inst_counts.zero_()
        self._updates = [0, 0]
        self._status_reset()
        return self
