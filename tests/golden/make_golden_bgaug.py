#!/usr/bin/env python
"""Golden fixture for the bg training augmentation, produced by the REFERENCE's transforms (build container only).

    python tests/golden/make_golden_bgaug.py

``RandomSizeAndCropMasks_Faster`` and ``RandomHorizontallyFlip`` (data/transforms.py:169-293) run unmodified, with the real
PIL, the way ``BGDataset`` chains them (data/datasets/bg_dataset.py:147-155,191-192: ``crop_nopad=False``, ``pre_size=None``,
``ignore_index=255``) on T = 3 label maps, one ground-truth map and one ``[H,W,T]`` array of u16 depth codes.  Stubs, in the
style of _ref_import.py: ``torchvision`` (imported, never used) and ``cv2``, which is not installed: ``cv2.resize`` below
restates OpenCV's published INTER_NEAREST rule (resize.cpp ``resizeNN``: ``sx = min(floor(x * (1/(dsize/ssize))), ssize-1)`` in
double, per axis), so the depth planes pin the pad / crop / flip bookkeeping of the arrays, NOT OpenCV's rounding.
``random`` is seeded per case; a recording proxy in front of the module notes what the transforms draw.

g12_bgaug.npz holds ``n_cases`` and per case ``c<i>_``:
  src_seg [3,H,W] u8, src_label [H,W] u8, src_depth [3,H,W] u16      the sources (H x W = 48 x 96 or 48 x 64)
  seed, scale_min, scale_max, size                                    what the case was run with (size 40)
  scale, x1, y1, flip                                                 what the transforms drew (x1 / y1 = -1: not drawn, i.e. 0)
  out_seg [3,40,40] u8, out_label [40,40] u8, out_depth [3,40,40] u16 the transformed planes
"""
import os
import random
import sys
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import REF_ROOT  # noqa: E402
SIZE, T = 40, 3

# (source h, source w, seed, scale_min, scale_max)
CASES = [
    (48, 96, 1, 0.8, 0.8),     # crop 32 (up-scaling); at 32, 48 and 64 PIL's accumulated index differs from the closed form
    (48, 96, 2, 1.2, 1.2),     # crop 48: h == crop (no y draw)
    (48, 96, 3, 1.6, 1.6),     # crop 64: pad in h only
    (48, 64, 4, 0.8, 0.8),     # crop 32
    (48, 64, 5, 1.2, 1.2),     # crop 48
    (48, 64, 6, 1.6, 1.6),     # crop 64: pad in h only, w == crop (no x draw)
    (48, 96, 7, 2.5, 2.5),     # crop 100: pad in both axes
    (48, 64, 8, 2.0, 2.0),     # crop 80: pad in both axes
    (48, 96, 9, 0.5, 2.0),     # the configured range of configs/bg/bg_train.yaml
    (48, 96, 10, 0.5, 2.0),
    (48, 64, 11, 0.5, 2.0),
    (48, 64, 12, 0.5, 2.0),
    (48, 96, 13, 1.0, 1.0),    # crop 40 == size: resize is the identity
]


def cv2_resize_standin(arr, dsize, interpolation=0):
    """cv2.resize(arr, dsize=(w, h), interpolation=INTER_NEAREST) by OpenCV's published rule (resizeNN)."""
    assert interpolation == 0
    w, h = dsize
    sh, sw = arr.shape[:2]
    xs = np.minimum(np.floor(np.arange(w) * (1.0 / (w / sw))).astype(np.int64), sw - 1)
    ys = np.minimum(np.floor(np.arange(h) * (1.0 / (h / sh))).astype(np.int64), sh - 1)
    return np.ascontiguousarray(arr[ys][:, xs])


class RecordingRandom:
    """Stands where the transforms module holds ``random``: delegates to the (seeded) module, notes every draw."""

    def __init__(self):
        self.calls = []

    def uniform(self, a, b):
        v = random.uniform(a, b)
        self.calls.append(('uniform', v))
        return v

    def randint(self, a, b):
        v = random.randint(a, b)
        self.calls.append(('randint', v, b))
        return v

    def random(self):
        v = random.random()
        self.calls.append(('random', v))
        return v


def install_stubs():
    for name, path in (('panoptic_forecasting', REF_ROOT + '/panoptic_forecasting'),
                       ('panoptic_forecasting.data', REF_ROOT + '/panoptic_forecasting/data')):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = [path]
            sys.modules[name] = m
    cv2 = types.ModuleType('cv2')
    cv2.INTER_NEAREST = 0
    cv2.setNumThreads = lambda n: None
    cv2.resize = cv2_resize_standin
    sys.modules['cv2'] = cv2
    if 'torchvision' not in sys.modules:
        sys.modules['torchvision'] = types.ModuleType('torchvision')
    sys.dont_write_bytecode = True  # the reference tree is read-only


def sources(h, w, seed):
    g = np.random.RandomState(1000 + seed)
    seg = g.randint(0, 19, (T, h, w)).astype(np.uint8)
    seg[g.rand(T, h, w) < 0.1] = 255
    label = g.randint(0, 19, (h, w)).astype(np.uint8)
    label[g.rand(h, w) < 0.1] = 255
    depth = g.randint(0, 65536, (T, h, w)).astype(np.uint16)
    depth[g.rand(T, h, w) < 0.2] = 0                # holes
    depth[:, 0, :4] = [[0, 255, 256, 257]] * T      # the codes either side of depth 0
    return seg, label, depth


def main():
    install_stubs()
    from panoptic_forecasting.data import transforms
    rec = RecordingRandom()
    transforms.random = rec
    arrs = {'n_cases': np.int64(len(CASES))}
    seen = set()
    for i, (h, w, seed, smin, smax) in enumerate(CASES):
        seg, label, depth = sources(h, w, seed)
        chain = [transforms.RandomSizeAndCropMasks_Faster(SIZE, False, pre_size=None, scale_min=smin, scale_max=smax,
                                                          ignore_index=255),
                 transforms.RandomHorizontallyFlip()]
        random.seed(seed)
        rec.calls = []
        segs, mask, arrs_ = [Image.fromarray(s) for s in seg], Image.fromarray(label), [np.moveaxis(depth, 0, 2).copy()]
        for tr in chain:
            segs, mask, arrs_ = tr(segs, mask, arrs_)
        calls = list(rec.calls)
        assert calls[0][0] == 'uniform' and calls[-1][0] == 'random'
        scale, flip = calls[0][1], calls[-1][1] < 0.5
        crop = int(SIZE * scale)
        ints = [c for c in calls if c[0] == 'randint']
        pad_w = (crop - w) // 2 + 1 if crop > w else 0
        pad_h = (crop - h) // 2 + 1 if crop > h else 0
        x_drawn, y_drawn = w + 2 * pad_w != crop, h + 2 * pad_h != crop
        assert len(ints) == int(x_drawn) + int(y_drawn)
        x1 = ints[0][1] if x_drawn else -1
        y1 = ints[-1][1] if y_drawn else -1
        p = 'c%d_' % i
        arrs[p + 'src_seg'], arrs[p + 'src_label'], arrs[p + 'src_depth'] = seg, label, depth
        arrs[p + 'seed'], arrs[p + 'size'] = np.int64(seed), np.int64(SIZE)
        arrs[p + 'scale_min'], arrs[p + 'scale_max'], arrs[p + 'scale'] = np.float64(smin), np.float64(smax), np.float64(scale)
        arrs[p + 'x1'], arrs[p + 'y1'], arrs[p + 'flip'] = np.int64(x1), np.int64(y1), np.bool_(flip)
        arrs[p + 'out_seg'] = np.stack([np.array(s) for s in segs]).astype(np.uint8)
        arrs[p + 'out_label'] = np.array(mask).astype(np.uint8)
        out_depth = np.ascontiguousarray(np.moveaxis(np.asarray(arrs_[0]), 2, 0))
        assert out_depth.dtype == np.uint16 and out_depth.shape == (T, SIZE, SIZE)
        arrs[p + 'out_depth'] = out_depth
        kind = ('pad_both' if pad_w and pad_h else 'pad_h' if pad_h else 'no_pad', bool(flip), 'down' if crop > SIZE else 'up')
        seen.add(kind)
        print('case %2d: %dx%d seed %2d scale %.4f crop %3d pad (%d,%d) x1 %3d y1 %3d flip %d' %
              (i, h, w, seed, scale, crop, pad_w, pad_h, x1, y1, flip))
    pads, flips = {k[0] for k in seen}, {k[1] for k in seen}
    assert pads == {'no_pad', 'pad_h', 'pad_both'} and flips == {True, False} and {k[2] for k in seen} == {'down', 'up'}, seen
    crops = {int(SIZE * float(arrs['c%d_scale' % i])) for i in range(len(CASES))}
    assert {32, 48, 64} <= crops, crops
    out = os.path.join(HERE, 'g12_bgaug.npz')
    np.savez_compressed(out, **arrs)
    print('wrote %s (%d bytes)' % (out, os.path.getsize(out)))


if __name__ == '__main__':
    main()
