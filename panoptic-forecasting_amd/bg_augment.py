"""Host side of the bg training augmentation (``pf_bg_augment``, csrc/bg_augment.hip).

The reference transforms every training sample of ``BGDataset`` with ``RandomSizeAndCropMasks_Faster`` and
``RandomHorizontallyFlip`` (``data/transforms.py:169-293``): a random scale, a constant pad where the crop exceeds the
source, a random crop, a nearest-neighbour resize to ``size`` and a random flip, applied jointly to T label maps, one
ground-truth map (PIL images) and the ``[H,W,T]`` depth codes (numpy, ``cv2.resize``).  Each of those steps acts on one axis
at a time, so the whole transform of one sample is four index tables:

    out[y][x] = src[y_tab[y]][x_tab[x]]        entry -1 = padding (255 in label maps, code 0 in depth)

``draw_params`` restates the random draws (same calls on a ``random.Random``, same order, same conditions), ``build_tables``
folds pad, crop, resize and flip into the tables, and the device kernel is a table-driven gather.  The tables are built on
the host because the two nearest-neighbour rules differ and neither is the textbook one:

  label maps   PIL ``Image.resize(size, NEAREST)`` walks the source coordinate by ACCUMULATION in double:
               ``xo = 0.5*a; idx = int(xo); xo += a`` with ``a = crop/size`` (Pillow, Geometry.c ``ImagingScaleAffine``).
               The closed form ``floor((x + 0.5)*a)`` differs from it, e.g. at crop 448, 512 ... 1152 -> 800.
  depth arrays ``cv2.resize(dsize=size, INTER_NEAREST)``: ``min(floor(x * (1/(size/crop))), crop - 1)`` in double (OpenCV,
               resize.cpp ``resizeNN``).  OpenCV is not installed where the fixtures are made: this rule is restated from
               its published source and is not pinned by a recorded output.
"""
import math

import numpy as np
import torch

from . import lib as _lib

PAD = -1     # table entry for "outside the source": any value outside [0, extent) is padding to the kernel


def _pair(size):
    """``size`` as the reference takes it: a number (square) or ``(w, h)`` — PIL's and cv2's ``dsize`` order."""
    if isinstance(size, (int, float)):
        return int(size), int(size)
    return int(size[0]), int(size[1])


def draw_params(rng, src_w, src_h, size, scale_min, scale_max):
    """``transforms.py:195-232`` (scale, pad, crop offsets; ``pre_size=None``) followed by ``:278`` (flip) on ``rng``."""
    size_w, size_h = _pair(size)
    scale = 1. * rng.uniform(scale_min, scale_max)
    crop_w, crop_h = int(size_w * scale), int(size_h * scale)
    pad_h = (crop_h - src_h) // 2 + 1 if crop_h > src_h else 0
    pad_w = (crop_w - src_w) // 2 + 1 if crop_w > src_w else 0
    w, h = src_w + 2 * pad_w, src_h + 2 * pad_h
    x1 = 0 if w == crop_w else rng.randint(0, w - crop_w)
    y1 = 0 if h == crop_h else rng.randint(0, h - crop_h)
    flip = rng.random() < 0.5
    return {'scale': scale, 'crop_w': crop_w, 'crop_h': crop_h, 'pad_w': pad_w, 'pad_h': pad_h, 'x1': x1, 'y1': y1, 'flip': flip}


def draw_flip(rng):
    """``data.no_resize_crop``: the flip alone (``bg_dataset.py:144-145``)."""
    return {'flip': rng.random() < 0.5}


def pil_nearest_index(crop, size):
    """Source index of every output index under PIL ``resize(NEAREST)`` of ``crop`` -> ``size`` samples."""
    a = crop / size
    out = np.empty(size, np.int64)
    xo = 0.5 * a
    for x in range(size):
        out[x] = int(xo)
        xo += a
    return out


def cv2_nearest_index(crop, size):
    """Source index of every output index under ``cv2.resize(INTER_NEAREST)`` of ``crop`` -> ``size`` samples."""
    ifx = 1. / (size / crop)
    return np.array([min(int(math.floor(x * ifx)), crop - 1) for x in range(size)], np.int64)


def _axis(index, crop, offset, pad, src):
    """Resized index -> source index: crop offset and pad folded in, everything outside the source marked ``PAD``."""
    idx = np.where((index >= 0) & (index < crop), index + offset - pad, PAD)
    return np.where((idx >= 0) & (idx < src), idx, PAD).astype(np.int32)


def build_tables(params, src_w, src_h, size):
    """(y_map [oh], x_map [ow], y_arr [oh], x_arr [ow]) int32 for one sample: ``*_map`` for the label maps, ``*_arr`` for the
    depth arrays.  ``params``: ``draw_params``' dict, ``draw_flip``'s (no resize, no crop: ``size`` is the source size) or
    ``None`` (validation: identity)."""
    if params is None or 'crop_w' not in params:
        ow, oh = src_w, src_h
        x = np.arange(ow, dtype=np.int32)
        y = np.arange(oh, dtype=np.int32)
        tabs = [y, x, y.copy(), x.copy()]
    else:
        ow, oh = _pair(size)
        cw, ch, pw, ph, x1, y1 = (params[k] for k in ('crop_w', 'crop_h', 'pad_w', 'pad_h', 'x1', 'y1'))
        tabs = [_axis(pil_nearest_index(ch, oh), ch, y1, ph, src_h), _axis(pil_nearest_index(cw, ow), cw, x1, pw, src_w),
                _axis(cv2_nearest_index(ch, oh), ch, y1, ph, src_h), _axis(cv2_nearest_index(cw, ow), cw, x1, pw, src_w)]
    if params is not None and params.get('flip'):
        tabs[1] = tabs[1][::-1]
        tabs[3] = tabs[3][::-1]
    return tuple(np.ascontiguousarray(t, dtype=np.int32) for t in tabs)


def gather_numpy(src, y_tab, x_tab, pad):
    """``out[..., y, x] = src[..., y_tab[y], x_tab[x]]`` with ``pad`` where either entry is outside the source: the host
    statement of what the kernel computes (tests, and the only consumer of the tables besides the kernel)."""
    h, w = src.shape[-2:]
    y_ok, x_ok = (y_tab >= 0) & (y_tab < h), (x_tab >= 0) & (x_tab < w)
    out = src[..., np.where(y_ok, y_tab, 0), :][..., np.where(x_ok, x_tab, 0)]
    out[..., ~y_ok, :] = pad
    out[..., ~x_ok] = pad
    return out


def device_augment(seg_src, label_src, depth_src, y_map, x_map, y_arr, x_arr, min_depth, max_depth, pad_label=255, out=None):
    """One ``pf_bg_augment`` launch on the current stream.  ``seg_src [B,T,Hs,Ws]`` u8, ``label_src [B,Hs,Ws]`` u8 | None,
    ``depth_src [B,T,Hs,Ws]`` 16-bit codes | None, tables ``[B,oh]`` / ``[B,ow]`` int32 — all on the device.  Returns
    ``(seg u8, label u8 | None, depth f32 | None, mask bool | None)``; ``out`` = the same 4-tuple (mask u8) to write into."""
    L = _lib.load()
    seg_src = _lib.require_cuda(seg_src, 'seg_src')
    if seg_src.dtype != torch.uint8 or seg_src.dim() != 4:
        raise _lib.PfError('seg_src must be [B,T,Hs,Ws] uint8 (got %s %s)' % (tuple(seg_src.shape), seg_src.dtype))
    b, t, hs, ws = seg_src.shape
    tabs = [y_map, x_map] + ([y_arr, x_arr] if depth_src is not None else [])
    for tab in tabs:
        _lib.require_cuda(tab, 'index table')
        if tab.dtype != torch.int32 or tab.dim() != 2 or tab.shape[0] != b:
            raise _lib.PfError('index tables must be [B,n] int32 (got %s %s)' % (tuple(tab.shape), tab.dtype))
    oh, ow = y_map.shape[1], x_map.shape[1]
    if depth_src is not None and (y_arr.shape[1] != oh or x_arr.shape[1] != ow):
        raise _lib.PfError('label-map and depth-array tables must have the same lengths')
    if label_src is not None:
        _lib.require_cuda(label_src, 'label_src')
        if label_src.dtype != torch.uint8 or tuple(label_src.shape) != (b, hs, ws):
            raise _lib.PfError('label_src must be [B,Hs,Ws] uint8 (got %s %s)' % (tuple(label_src.shape), label_src.dtype))
    if depth_src is not None:
        _lib.require_cuda(depth_src, 'depth_src')
        if depth_src.element_size() != 2 or tuple(depth_src.shape) != (b, t, hs, ws):
            raise _lib.PfError('depth_src must be [B,T,Hs,Ws] 16-bit codes (got %s %s)' % (tuple(depth_src.shape), depth_src.dtype))
    dev = seg_src.device
    if out is None:
        out = (torch.empty((b, t, oh, ow), dtype=torch.uint8, device=dev),
               torch.empty((b, oh, ow), dtype=torch.uint8, device=dev) if label_src is not None else None,
               torch.empty((b, t, oh, ow), dtype=torch.float32, device=dev) if depth_src is not None else None,
               torch.empty((b, t, oh, ow), dtype=torch.uint8, device=dev) if depth_src is not None else None)
    o_seg, o_lab, o_dep, o_msk = out
    ptr = lambda x: x.data_ptr() if x is not None else None      # noqa: E731
    _lib.check(L.pf_bg_augment(ptr(seg_src), ptr(label_src), ptr(depth_src), b, t, hs, ws, ptr(y_map), ptr(x_map),
                               ptr(y_arr) if depth_src is not None else None, ptr(x_arr) if depth_src is not None else None,
                               oh, ow, int(pad_label), float(min_depth), float(max_depth), ptr(o_seg), ptr(o_lab), ptr(o_dep),
                               ptr(o_msk), _lib.stream_ptr()), 'pf_bg_augment')
    return o_seg, o_lab, o_dep, (o_msk.view(torch.bool) if o_msk is not None else None)
