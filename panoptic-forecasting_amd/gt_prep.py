"""Cityscapes ground-truth preparation from the instance maps (``*_gtFine_instanceIds.png``): the panoptic PNG's pixels and segment
list of ``cityscapesscripts.preparation.createPanopticImgs``, the trainId map of ``createTrainIdLabelImgs`` and the trainId map
without the thing classes of the reference's ``scripts/preprocessing/remove_fg_from_gt.py``.  cityscapesscripts is absent here and its
version unpinned: the rules are written down in include/pfhip.h (pf_gt_prepare block) from the originals as remembered; parity with
them is unpinned.  ``remove_fg_host`` is held against the reference's own script by fixture G14.

A value v of an instance map is a labelId when below 1000, else labelId * 1000 + instance index.  ``GTPreparer.prepare`` enqueues the
HIP kernels (csrc/gt_prepare.hip), ``prepare_host`` states the same in numpy for a machine without a GPU, and tests/gtprep_ref.py
restates it a third time per segment, without either.
"""
from collections import namedtuple

import numpy as np
import torch

from . import lib as _lib
from .meter import DeviceMeter

Label = namedtuple('Label', 'name id train_id category category_id has_instances ignore_in_eval color')

# the public Cityscapes label table (csrc/gt_labels.h is the device side's copy; tests/test_gt_prep_host.py compares the two)
LABELS = (
    Label('unlabeled', 0, 255, 'void', 0, False, True, (0, 0, 0)),
    Label('ego vehicle', 1, 255, 'void', 0, False, True, (0, 0, 0)),
    Label('rectification border', 2, 255, 'void', 0, False, True, (0, 0, 0)),
    Label('out of roi', 3, 255, 'void', 0, False, True, (0, 0, 0)),
    Label('static', 4, 255, 'void', 0, False, True, (0, 0, 0)),
    Label('dynamic', 5, 255, 'void', 0, False, True, (111, 74, 0)),
    Label('ground', 6, 255, 'void', 0, False, True, (81, 0, 81)),
    Label('road', 7, 0, 'flat', 1, False, False, (128, 64, 128)),
    Label('sidewalk', 8, 1, 'flat', 1, False, False, (244, 35, 232)),
    Label('parking', 9, 255, 'flat', 1, False, True, (250, 170, 160)),
    Label('rail track', 10, 255, 'flat', 1, False, True, (230, 150, 140)),
    Label('building', 11, 2, 'construction', 2, False, False, (70, 70, 70)),
    Label('wall', 12, 3, 'construction', 2, False, False, (102, 102, 156)),
    Label('fence', 13, 4, 'construction', 2, False, False, (190, 153, 153)),
    Label('guard rail', 14, 255, 'construction', 2, False, True, (180, 165, 180)),
    Label('bridge', 15, 255, 'construction', 2, False, True, (150, 100, 100)),
    Label('tunnel', 16, 255, 'construction', 2, False, True, (150, 120, 90)),
    Label('pole', 17, 5, 'object', 3, False, False, (153, 153, 153)),
    Label('polegroup', 18, 255, 'object', 3, False, True, (153, 153, 153)),
    Label('traffic light', 19, 6, 'object', 3, False, False, (250, 170, 30)),
    Label('traffic sign', 20, 7, 'object', 3, False, False, (220, 220, 0)),
    Label('vegetation', 21, 8, 'nature', 4, False, False, (107, 142, 35)),
    Label('terrain', 22, 9, 'nature', 4, False, False, (152, 251, 152)),
    Label('sky', 23, 10, 'sky', 5, False, False, (70, 130, 180)),
    Label('person', 24, 11, 'human', 6, True, False, (220, 20, 60)),
    Label('rider', 25, 12, 'human', 6, True, False, (255, 0, 0)),
    Label('car', 26, 13, 'vehicle', 7, True, False, (0, 0, 142)),
    Label('truck', 27, 14, 'vehicle', 7, True, False, (0, 0, 70)),
    Label('bus', 28, 15, 'vehicle', 7, True, False, (0, 60, 100)),
    Label('caravan', 29, 255, 'vehicle', 7, True, True, (0, 0, 90)),
    Label('trailer', 30, 255, 'vehicle', 7, True, True, (0, 0, 110)),
    Label('train', 31, 16, 'vehicle', 7, True, False, (0, 80, 100)),
    Label('motorcycle', 32, 17, 'vehicle', 7, True, False, (0, 0, 230)),
    Label('bicycle', 33, 18, 'vehicle', 7, True, False, (119, 11, 32)),
    Label('license plate', -1, -1, 'vehicle', 7, False, True, (0, 0, 142)),
)
ID2LABEL = {l.id: l for l in LABELS}
N_IDS = 34                                    # every labelId of an instance map is below this
MOVING_TRAIN_IDS = tuple(l.train_id for l in LABELS if l.has_instances and not l.ignore_in_eval)   # remove_fg_from_gt.py's list

STATUS_BITS = ((1, 'PF_GTPREP_STATUS_FULL: an image has more listed segments than the list holds'),
               (2, 'PF_GTPREP_STATUS_VALUE: an instance-map value outside [0, 34) and [1000, 34000)'))
WANT = ('panoptic', 'trainids', 'nofg')
_KINDS = {torch.int32: 1, torch.int64: 2}     # any 2-byte integer tensor is read as u16: kind 0

_TRAIN_LUT = np.full(N_IDS, 255, np.uint8)
_LISTED = np.zeros(N_IDS, bool)
for _l in LABELS:
    if _l.id >= 0:
        _TRAIN_LUT[_l.id] = _l.train_id
        _LISTED[_l.id] = not _l.ignore_in_eval
_NOFG_LUT = np.arange(256, dtype=np.uint8)
_NOFG_LUT[list(MOVING_TRAIN_IDS)] = 255


def max_segments():
    return _lib.load().pf_gt_prepare_max_segments()


def _check_want(want):
    want = tuple(want)
    bad = [w for w in want if w not in WANT]
    if bad or not want:
        raise _lib.PfError('gt_prep: want must name some of %s (got %s)' % (WANT, want))
    return want


def remove_fg_host(trainid_map):
    """remove_fg_from_gt.py's rule as one 256-entry lookup: the trainIds of the labels with instances that are evaluated -> 255."""
    arr = np.asarray(trainid_map)
    if arr.dtype != np.uint8:
        raise _lib.PfError('remove_fg_host: a trainId map is 8-bit (got %s)' % arr.dtype)
    return _NOFG_LUT[arr]


def _as_values(inst):
    """Host maps as int64 [B,H,W]; a 2-byte integer map is read as u16 (as the device reads it)."""
    arr = np.asarray(inst)
    if arr.dtype.kind not in 'iu':
        raise _lib.PfError('gt_prep: an instance map holds integers (got %s)' % arr.dtype)
    if arr.dtype.itemsize == 2:
        arr = arr.view(np.uint16)
    if arr.ndim == 2:
        arr = arr[None]
    if arr.ndim != 3:
        raise _lib.PfError('gt_prep: instance maps are [B,H,W] or [H,W] (got %s)' % (arr.shape,))
    if arr.dtype == np.uint64:
        if (arr >> np.uint64(63)).any():
            raise _lib.PfError('gt_prep: %s' % STATUS_BITS[1][1])
    return arr.astype(np.int64)


def prepare_host(inst, want=WANT):
    """``GTPreparer.prepare`` on the host, in numpy: {'panoptic' [B,H,W,3] u8, 'trainids' [B,H,W] u8, 'nofg' [B,H,W] u8, 'seg_count'
    [B] i32, 'segs' [B,max_segments,6] i32} (the segment list comes with 'panoptic').  An image with an illegal value or with more
    segments than the list holds raises PfError naming the status bit and the image."""
    want = _check_want(want)
    vals = _as_values(inst)
    b, h, w = vals.shape
    cap = max_segments()
    legal = ((vals >= 0) & (vals < N_IDS)) | ((vals >= 1000) & (vals < N_IDS * 1000))
    if not legal.all():
        where = np.argwhere(~legal)[0]
        raise _lib.PfError('gt_prep status 2: %s (image %d of the batch: value %d at row %d, column %d)'
                           % (STATUS_BITS[1][1], where[0], vals[tuple(where)], where[1], where[2]))
    label = np.where(vals < 1000, vals, vals // 1000)
    train = _TRAIN_LUT[label]
    out = {}
    if 'trainids' in want:
        out['trainids'] = train
    if 'nofg' in want:
        out['nofg'] = _NOFG_LUT[train]
    if 'panoptic' in want:
        col = np.where(_LISTED[label], vals, 0)
        out['panoptic'] = np.stack([col % 256, col // 256 % 256, col // 65536], -1).astype(np.uint8)
        out['seg_count'] = np.zeros(b, np.int32)
        out['segs'] = np.zeros((b, cap, 6), np.int32)
        for i in range(b):
            flat = vals[i].ravel()
            order = np.argsort(flat, kind='stable')
            sv = flat[order]
            starts = np.flatnonzero(np.concatenate(([True], sv[1:] != sv[:-1])))
            ids = sv[starts]
            area = np.diff(np.concatenate((starts, [flat.size])))
            xs, ys = order % w, order // w
            x0, x1 = np.minimum.reduceat(xs, starts), np.maximum.reduceat(xs, starts)
            y0, y1 = np.minimum.reduceat(ys, starts), np.maximum.reduceat(ys, starts)
            keep = _LISTED[np.where(ids < 1000, ids, ids // 1000)]
            rows = np.stack([ids, area, x0, y0, x1 - x0 + 1, y1 - y0 + 1], 1)[keep]
            if len(rows) > cap:
                raise _lib.PfError('gt_prep status 1: %s (image %d of the batch: %d segments, the list holds %d)'
                                   % (STATUS_BITS[0][1], i, len(rows), cap))
            out['seg_count'][i] = len(rows)
            out['segs'][i, :len(rows)] = rows
    return out


def segment_rows(result):
    """The [n,6] int rows {v, area, x, y, width, height} of each image of a ``prepare`` / ``prepare_host`` result, on the host."""
    count, segs = result['seg_count'], result['segs']
    if isinstance(count, torch.Tensor):
        count, segs = count.cpu().numpy(), segs.cpu().numpy()
    return [np.array(segs[b, :int(count[b])]) for b in range(len(count))]


def segments_info(rows, use_train_id=False):
    """createPanopticImgs' dicts of one image from its rows: iscrowd is 1 exactly for a thing label without an instance part;
    category_id is the labelId, or the trainId with ``use_train_id``."""
    out = []
    for v, area, x, y, w, h in (map(int, r) for r in rows):
        label = ID2LABEL[v if v < 1000 else v // 1000]
        out.append({'id': v, 'category_id': label.train_id if use_train_id else label.id, 'area': area, 'bbox': [x, y, w, h],
                    'iscrowd': int(v < 1000 and label.has_instances)})
    return out


def categories(use_train_id=False):
    """The 'categories' of the panoptic JSON: every label that is evaluated."""
    return [{'id': l.train_id if use_train_id else l.id, 'name': l.name, 'color': list(l.color), 'supercategory': l.category,
             'isthing': int(l.has_instances)} for l in LABELS if not l.ignore_in_eval]


class GTPreparer(DeviceMeter):
    """Holds the workspace of pf_gt_prepare and its sticky status word (meter.py's rules: the workspace may not grow during a
    graph capture or after one)."""
    WORKSPACES = {'gt_prepare': ('_ws', '')}
    HOST_PATH = 'gt_prep.prepare_host'
    ENQUEUE = 'prepare'

    def __init__(self, device='cuda'):
        super().__init__(device)
        self.max_segments = max_segments()

    @torch.no_grad()
    def prepare(self, inst, want=WANT, out=None, check=True):
        """inst [B,H,W] (or [H,W]) on the device: a 2-byte integer tensor (read as u16), int32 or int64.  Returns the device
        tensors {'panoptic' [B,H,W,3] u8, 'trainids' [B,H,W] u8, 'nofg' [B,H,W] u8, 'seg_count' [B] i32, 'segs'
        [B,max_segments,6] i32}: those named in ``want`` ('seg_count' and 'segs' come with 'panoptic'; rows past seg_count are not
        written).  ``out`` may hold tensors to write into.  Only enqueues; then, unless ``check`` is false or a graph is being
        captured, waits and raises PfError naming the status bit (``check()`` does the same later)."""
        lib = self._lib
        want = _check_want(want)
        if inst.dim() == 2:
            inst = inst[None]
        if inst.dim() != 3:
            raise lib.PfError('GTPreparer: instance maps are [B,H,W] or [H,W] (got %s)' % (tuple(inst.shape),))
        if inst.dtype.is_floating_point or inst.dtype == torch.bool or (inst.element_size() != 2 and inst.dtype not in _KINDS):
            raise lib.PfError('GTPreparer: an instance map is a 16-bit, int32 or int64 tensor (got %s)' % inst.dtype)
        lib.require_cuda(inst, 'inst')
        b, h, w = inst.shape
        shapes = {'panoptic': ((b, h, w, 3), torch.uint8), 'trainids': ((b, h, w), torch.uint8), 'nofg': ((b, h, w), torch.uint8),
                  'seg_count': ((b,), torch.int32), 'segs': ((b, self.max_segments, 6), torch.int32)}
        names = [n for n in WANT if n in want] + (['seg_count', 'segs'] if 'panoptic' in want else [])
        res = {}
        for name in names:
            shape, dtype = shapes[name]
            t = out.get(name) if out else None
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=inst.device)
            elif tuple(t.shape) != shape or t.dtype != dtype or t.device != inst.device:
                raise lib.PfError('GTPreparer: out[%r] must be %s %s on %s' % (name, shape, dtype, inst.device))
            res[name] = lib.require_cuda(t, 'out[%r]' % name)
        ptr = lambda name: res[name].data_ptr() if name in res else None
        if b:
            ws = self._workspace(b, 'gt_prepare')
            lib.check(lib.load().pf_gt_prepare(inst.data_ptr(), _KINDS.get(inst.dtype, 0), b, h, w, ptr('panoptic'), ptr('trainids'),
                                               ptr('nofg'), ptr('seg_count'), ptr('segs'), ws.data_ptr(), ws.numel(),
                                               lib.stream_ptr()), 'pf_gt_prepare')
        if check and not torch.cuda.is_current_stream_capturing():
            self.check()
        return res

    def status(self):
        """The sticky status word (waits for the current stream)."""
        return self._status_word('gt_prepare')

    def status_async(self):
        """A pinned host int32 [1] that receives the status word as it stands after everything enqueued so far: the copy is enqueued
        on the current stream and nothing waits.  Read it after an event recorded behind this call; ``raise_for`` names its bits."""
        word = torch.zeros(1, dtype=torch.int32).pin_memory()
        if self._ws is not None:
            word.copy_(self._ws[:4].view(torch.int32), non_blocking=True)
        return word

    def raise_for(self, st):
        if st:
            raise self._lib.PfError('gt_prep status %d: %s (a flagged image lists no segments; reset() clears this)'
                                    % (st, '; '.join(text for bit, text in STATUS_BITS if st & bit)))

    def check(self):
        self.raise_for(self.status())

    def reset(self):
        self._status_reset()
        return self
