"""Semantic confusion matrix, IoU and mIoU for label maps: the semantics of include/pfhip.h's pf_confusion_accumulate block.

The reference leaves the scoring of its semantic outputs (the bg forecast of ``export_bg.py``, ``FGModel.predict_semantics``) to the
external ``cityscapesscripts.evaluation.evalPixelLevelSemanticLabeling``; that package is absent here and its version unpinned, so
the formula below is written down from the Cityscapes pixel-level evaluator as remembered: parity unpinned.
iIoU (instance-weighted) is not built: it needs instance ids and the evaluator's class-size table.

``confusion_host`` states the counting in torch (any device; the host path of eval_semantic.py); ``SemanticIoU`` enqueues the HIP
kernels (csrc/confusion_kernels.hip); tests/conf_ref64.py restates both a third time, without either.

A confusion table is [20,20] int64: row = ground-truth class, column = predicted class, index 19 = void.  Integers add exactly, so
a sharded evaluation reproduces the single-process table bit for bit.
"""
import torch

FORMATS = {'trainid': 0, 'cityscapes': 1}
N_CELLS = 20                           # 19 classes + void
VOID = 19
FIRST_MO = 11                          # trainIds 0..10 are stuff, 11..18 the moving objects
STATUS_BITS = ((1, 'PF_CONF_STATUS_VALUE: a label value outside [0, 256)'),)
_KINDS = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}


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


class SemanticIoU:
    """Device-side confusion meter: ``update`` enqueues pf_confusion_accumulate on the current stream and returns at once (no
    synchronisation, capturable), ``acc`` is the [20,20] int64 device tensor, ``result`` waits and reads the status word."""

    def __init__(self, n_cls=19, fmt='trainid', device='cuda'):
        from . import lib as _lib
        if fmt not in FORMATS:
            raise ValueError('fmt must be one of %s (got %r)' % (sorted(FORMATS), fmt))
        if not 1 <= n_cls <= 19:
            raise ValueError('n_cls must be 1..19')
        self._lib = _lib
        self.n_cls, self.fmt = n_cls, fmt
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.PfError('SemanticIoU runs on the GPU (got %s): use confusion_host on the host' % self.device)
        self.acc = torch.zeros(N_CELLS, N_CELLS, dtype=torch.int64, device=self.device)
        self._ws = None
        self._captured = False

    def _workspace(self, b):
        """The workspace grows with the largest B seen.  A captured graph keeps the pointer it was captured with, so the
        workspace may not grow during a capture or after one: call update once with the largest batch before capturing."""
        import ctypes
        need = ctypes.c_size_t()
        self._lib.check(self._lib.load().pf_confusion_workspace(b, ctypes.byref(need)), 'pf_confusion_workspace')
        capturing = torch.cuda.is_current_stream_capturing()
        if self._ws is None or self._ws.numel() < need.value:
            if capturing or self._captured:
                raise self._lib.PfError('SemanticIoU: the workspace would have to grow to B = %d %s a graph capture, whose replays '
                                        'keep the old pointer: call update() with the largest batch before capturing'
                                        % (b, 'during' if capturing else 'after'))
            ws = torch.zeros(need.value, dtype=torch.uint8, device=self.device)    # status word starts at 0
            if self._ws is not None:
                ws[:256].copy_(self._ws[:256])                                       # a sticky bit survives the growth
            self._ws = ws
        self._captured = self._captured or capturing
        return self._ws

    @torch.no_grad()
    def update(self, pred, gt, per_image=None):
        """pred, gt [B,H,W] u8, i32 or i64, passed as they are, each in its own width (i8 and i16 are widened to i32 on the device;
        any other dtype is refused); per_image: optional [B,20,20] int64 device tensor that receives each image's table."""
        L, lib = self._lib.load(), self._lib
        if pred.dim() != 3 or pred.shape != gt.shape:
            raise lib.PfError('pred and gt must be [B,H,W] of one shape (got %s and %s)' % (tuple(pred.shape), tuple(gt.shape)))
        maps = []
        for t, name in ((pred, 'pred'), (gt, 'gt')):
            lib.require_cuda(t, name)
            if t.dtype not in _KINDS and t.dtype not in (torch.int8, torch.int16):
                raise lib.PfError('%s must be an integer label map (got %s)' % (name, t.dtype))
            maps.append(t if t.dtype in _KINDS else t.to(torch.int32))
        b, h, w = pred.shape
        if b == 0:
            return self
        if h == 0 or w == 0:
            raise lib.PfError('pred and gt must hold pixels (got %s)' % (tuple(pred.shape),))
        if per_image is not None:
            lib.require_cuda(per_image, 'per_image')
            if per_image.dtype != torch.int64 or tuple(per_image.shape) != (b, N_CELLS, N_CELLS):
                raise lib.PfError('per_image must be int64 [%d,%d,%d]' % (b, N_CELLS, N_CELLS))
        ws = self._workspace(b)
        lib.check(L.pf_confusion_accumulate(maps[0].data_ptr(), _KINDS[maps[0].dtype], maps[1].data_ptr(), _KINDS[maps[1].dtype],
                                            FORMATS[self.fmt], self.n_cls, b, h, w, self.acc.data_ptr(),
                                            per_image.data_ptr() if per_image is not None else None,
                                            ws.data_ptr(), ws.numel(), lib.stream_ptr()), 'pf_confusion_accumulate')
        return self

    def status(self):
        """The sticky status word (waits for the current stream)."""
        import ctypes
        if self._ws is None:
            return 0
        st = ctypes.c_int()
        self._lib.check(self._lib.load().pf_confusion_status(self._ws.data_ptr(), self._lib.stream_ptr(), ctypes.byref(st)),
                        'pf_confusion_status')
        return st.value

    def result(self):
        """iou_from_confusion's dict; PfError naming the bit when the status word is set."""
        st = self.status()
        if st:
            raise self._lib.PfError('semantic IoU status %d: %s (the flagged images were left out of acc; reset() clears this)'
                                    % (st, '; '.join(text for bit, text in STATUS_BITS if st & bit)))
        return iou_from_confusion(self.acc)

    def reset(self):
        self.acc.zero_()
        if self._ws is not None:
            self._lib.check(self._lib.load().pf_confusion_status_reset(self._ws.data_ptr(), self._lib.stream_ptr()),
                            'pf_confusion_status_reset')
        return self
