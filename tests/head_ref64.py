"""Test helper for the upsample + argmax head and the fused validation loss (not a test module; CPU only, imports no GPU code): a
float64 reference that uses the contract's fp32 COORDINATES, the error bar that follows from it, and the cases both
tests/test_head_host.py and tests/test_gpu_head.py run.

The contract (csrc/conv_epilogue.h: lin_coord, the arithmetic of ATen's align_corners=True) computes the source coordinate of an
output index in fp32: scale = float(n_in - 1) / float(n_out - 1), r = scale * float(o) rounded to fp32, i0 = min(int(r), n_in - 1),
l1 = clamp(r - i0, 0, 1), l0 = 1 - l1.  ``coords`` restates that word for word in numpy fp32 scalars, so i0 / i1 / l0 / l1 are the
very numbers a correct kernel holds.  ``upsample64`` then forms v = hy0*(lx0*a + lx1*b) + hy1*(lx0*c + lx1*d) with those fp32
weights and the fp32 taps widened to float64: products of two 24-bit numbers are exact in float64, the three sums round at 2^-53.
What separates a correct fp32 kernel from this reference is therefore the rounding of its own six products and three sums only.

HEAD_BAR, derived.  u = 2^-24 (unit roundoff of fp32, round to nearest), M = max |tap| of the case.  A kernel computes
t0 = fl(fl(lx0*a) + fl(lx1*b)): each product is off by at most u*|product|, the sum by at most u*|sum|, and
|lx0*a| + |lx1*b| <= (lx0 + lx1)*M with lx0 + lx1 = 1 +- u, so |t0 - t0_exact| <= 2*u*M to first order; likewise t1.
v = fl(fl(hy0*t0) + fl(hy1*t1)): the errors of t0 and t1 arrive weighted by hy0 + hy1 = 1 +- u (2*u*M), the two products add
u*M, the sum u*M.  |v_fp32 - v64| <= 4*u*M to first order; HEAD_BAR = 4.5*u*M, the half covers the second-order terms (u^2*M*O(10))
and float64's own rounding.  A fused multiply-add removes one rounding and only lowers the error.  fp32 ATen on the CPU measures
0 .. 2.2 u*M over the cases below (tests/test_head_host.py); interpolation with float64 coordinates is up to 273 u*M away.

A pixel whose float64 top-1 / top-2 margin is <= 2*HEAD_BAR may legitimately get either label from an fp32 kernel (each of the two
logits moves by at most HEAD_BAR); everywhere else the label is determined.  NEAR_TIE_CAP bounds the share of such pixels.

LOSS_P, the per-pixel bound of the loss, derived.  The kernel (csrc/head_kernels.hip: seg_loss_tile_kernel) computes, on its fp32
logits v (each within HEAD_BAR of v64), nll = (best + logf(sum_c expf(v_c - best))) - v_label, converts to double and adds in
double.  log-sum-exp moves by at most max_c |dv_c|, so the interpolation enters twice: 2*HEAD_BAR (once through the log-sum-exp,
once through v_label).  On top, with the device functions' documented 1 ulp = 2*u relative error for expf and logf (HIP math API):
  v_c - best: one rounding, <= u*2M absolute, = relative in expf's value;  expf: 2*u relative;  the C-term fp32 sum: (C-1)*u
  relative  ->  the sum (in [1, C]) is off by at most (2M + 2 + C - 1)*u relative = absolute in its logarithm;
  logf: 2*u * ln C;  best + log: u*(M + ln C);  minus v_label: u*(2M + ln C).
Sum: LOSS_P = 2*HEAD_BAR + u*(5*M + C + 1 + 4*ln C), plus valid * 2^-53 * (2M + ln C) for the double accumulation of `valid` terms.
"""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
NEAR_TIE_CAP = 0.0005          # share of pixels with margin <= 2*HEAD_BAR, per case


def coords(n_in, n_out):
    """lin_coord for o = 0 .. n_out-1: (i0, i1: int64 arrays; l0, l1: float32 arrays)"""
    f32 = np.float32
    scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    r = scale * np.arange(n_out).astype(f32)                    # fp32 product, rounded to fp32
    assert r.dtype == np.float32
    i0 = np.minimum(r.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = np.clip(r - i0.astype(f32), f32(0), f32(1))
    l0 = f32(1) - l1
    assert l0.dtype == np.float32 and l1.dtype == np.float32
    return i0, i1, l0, l1


def head_bar(x):
    return 4.5 * U * float(x.abs().max())


def loss_p(m, c, valid):
    return 2 * 4.5 * U * m + U * (5 * m + c + 1 + 4 * math.log(c)) + valid * 2.0 ** -53 * (2 * m + math.log(c))


def upsample64(x, ho, wo, bump_col=None):
    """x: [B, C, Hin, Win] float32 -> [B, C, ho, wo] float64.  ``bump_col``: the deliberate error of tests/test_head_host.py - that
    output column reads its first tap one source column to the right"""
    assert x.dtype == torch.float32
    _, _, hin, win = x.shape
    y0, y1, hy0, hy1 = coords(hin, ho)
    x0, x1, lx0, lx1 = coords(win, wo)
    if bump_col is not None:
        x0 = x0.copy()
        x0[bump_col] = min(x0[bump_col] + 1, win - 1)
    y0, y1, x0, x1 = (torch.from_numpy(i) for i in (y0, y1, x0, x1))
    hy0, hy1 = (torch.from_numpy(w).double().view(1, 1, ho, 1) for w in (hy0, hy1))
    lx0, lx1 = (torch.from_numpy(w).double().view(1, 1, 1, wo) for w in (lx0, lx1))
    xd = x.double()
    top, bot = xd[:, :, y0], xd[:, :, y1]
    t0 = lx0 * top[:, :, :, x0] + lx1 * top[:, :, :, x1]
    t1 = lx0 * bot[:, :, :, x0] + lx1 * bot[:, :, :, x1]
    return hy0 * t0 + hy1 * t1


def argmax_first(v, last=False):
    """first maximum wins: a channel replaces the running best only if strictly greater (``last``: greater or equal - the rule the
    kernels must NOT follow, for tests/test_head_host.py)"""
    best = v[:, 0].clone()
    arg = torch.zeros(best.shape, dtype=torch.int64)
    for c in range(1, v.shape[1]):
        m = (v[:, c] >= best) if last else (v[:, c] > best)
        arg[m] = c
        best = torch.where(m, v[:, c], best)
    return arg


def margin(v):
    """top-1 minus top-2 per pixel"""
    t = v.topk(2, dim=1).values
    return t[:, 0] - t[:, 1]


def seg_loss64(logits, labels, ho, wo, ignore, v=None):
    """(sum of nll, valid pixels, correct pixels) of cross entropy on the upsampled logits in float64; labels equal to ``ignore``,
    < 0 or >= C are skipped (include/pfhip.h, seg_loss_tile_kernel).  ``v``: upsample64(logits, ho, wo) if the caller has it"""
    v = upsample64(logits, ho, wo) if v is None else v
    c = v.shape[1]
    lab = labels.long()
    valid = (lab != ignore) & (lab >= 0) & (lab < c)
    lsm = torch.log_softmax(v, 1)
    nll = -lsm.gather(1, lab.clamp(0, c - 1).unsqueeze(1)).squeeze(1)
    correct = (argmax_first(v) == lab) & valid
    return float(nll[valid].sum()), int(valid.sum()), int(correct.sum())


# ------------------------------------------------------------------------------------------------ the cases
class HeadCase:
    """C classes, Hin x Win -> Hout x Wout at batch B, and the kernel launch_head's conditions (csrc/net_select.cpp: choose_head) select"""

    def __init__(self, c, hin, win, ho, wo, kernel, note, b=2):
        self.c, self.hin, self.win, self.ho, self.wo, self.kernel, self.note, self.b = c, hin, win, ho, wo, kernel, note, b
        self.name = 'C%d %dx%d->%dx%d' % (c, hin, win, ho, wo)

    @property
    def seed(self):
        return 7000 + self.c * 1009 + self.hin * 131 + self.win * 17 + self.ho * 5 + self.wo

    def logits(self):
        """seeded randn * 3, [B, C, Hin, Win] float32 (a function of the case alone)"""
        g = torch.Generator().manual_seed(self.seed)
        return torch.randn(self.b, self.c, self.hin, self.win, generator=g) * 3

    def labels(self, ho=None, wo=None):
        """int64: randint(0, C + 1) with C -> 255 (ignored); a patch of 200 in the last image: out of range, not the ignore value, to
        be skipped; -1 and -100 (torch's default ignore value) in its first row: negative, to be skipped; image 0: every label
        ignored.  ``labels_u8`` is the same with the negative entries as 255"""
        ho, wo = ho or self.ho, wo or self.wo
        g = torch.Generator().manual_seed(self.seed + 1)
        lab = torch.randint(0, self.c + 1, (self.b, ho, wo), generator=g)
        lab[lab == self.c] = 255
        lab[-1, ho // 4:ho // 2 + 1, wo // 5:wo // 2 + 1] = 200
        lab[-1, 0, 0:wo:7] = -1
        lab[-1, 0, 3:wo:7] = -100
        lab[0] = 255
        return lab

    def labels_u8(self):
        lab = self.labels()
        lab[lab < 0] = 255
        return lab.to(torch.uint8)


def _col(c):
    return 'head_col_kernel<%d>' % c


HEAD_COL_SHAPES = [
    (16, 80, 64, 320, "the workload's ratio; two column tiles, the second one partial"),
    (18, 75, 70, 300, 'non-integer ratio; the last row tile has 6 of 32 rows'),
    (9, 40, 72, 320, '8x'),
    # 2x: 18 x 130 source pixels per tile and channel, 103 KB at 11 classes - the window does NOT fit, launch_head falls back
    (35, 150, 70, 300, '2x: the window of head_col exceeds 60 KB; Wout % 4 == 0 but 3*sw > 1'),
    (2, 2, 33, 257, 'the smallest source; one lane in the second column tile, one row in the second row tile'),
    # an integer ratio of 2 that DOES fit the tiled head: 2x in width (130 source columns per tile) at 3 source rows per tile
    (2, 150, 40, 300, '2x in width on the tiled head (3 x 130 source pixels per tile); 8 of 32 rows in the last row tile'),
]
HEAD_CASES = [HeadCase(c, hi, wi, ho, wo, 'head_kernel' if (hi, wi) == (35, 150) else _col(c), note)
              for c in (11, 19) for hi, wi, ho, wo, note in HEAD_COL_SHAPES]
HEAD_CASES += [
    HeadCase(5, 9, 13, 33, 40, 'head4_kernel', '3*sw = 0.92: 4 outputs straddle 3 source columns'),
    HeadCase(11, 200, 13, 34, 40, 'head4_kernel', "head_col's LDS window does not fit: the fallback"),
    HeadCase(11, 1, 13, 5, 40, 'head4_kernel', 'Hin = 1'),
    HeadCase(5, 9, 13, 33, 41, 'head_kernel', 'Wout % 4 != 0'),
    HeadCase(5, 9, 14, 33, 40, 'head_kernel', '3*sw rounds to 1.0 in fp32: the condition of head4 is just missed'),
    HeadCase(11, 20, 30, 20, 30, 'head_kernel', 'identity: all weights exactly 0 or 1; the window of head_col does not fit'),
    HeadCase(11, 64, 128, 32, 64, 'head_kernel', 'downsampling; the window of head_col does not fit'),
    HeadCase(11, 13, 1, 40, 8, 'head_kernel', 'Win = 1'),
    # both scales 0.  With 11 classes, a source of at least 2 x 2 and a 3 x 3 window the conditions of launch_head select the
    # TILED head (rows = cols = 2 of its window are staged, all weight on the first); the 5-class twin reaches head_kernel
    HeadCase(11, 9, 13, 1, 1, _col(11), 'both scales 0 (tiled head: C = 11, Hin, Win >= 2, the window fits)'),
    HeadCase(5, 9, 13, 1, 1, 'head_kernel', 'both scales 0'),
]
# fp32 coordinates are exact here (scale 0, 1 or a power of two), so float64 coordinates give the same result
EXACT_COORDS = {'C11 20x30->20x30', 'C11 9x13->1x1', 'C5 9x13->1x1', 'C11 2x2->33x257', 'C19 2x2->33x257'}

LOSS_CASES = [HeadCase(c, hi, wi, ho, wo, 'seg_loss_tile_kernel<%d>' % c, note) for c in (11, 19) for hi, wi, ho, wo, note in HEAD_COL_SHAPES[:3]]
# 5 x 17 x 4 = 340 partial sums: the n > 256 loop of seg_loss_finish_kernel
LOSS_CASES += [HeadCase(c, 68, 258, 272, 1030, 'seg_loss_tile_kernel<%d>' % c, '340 workgroups', b=4) for c in (11, 19)]


@functools.lru_cache(maxsize=None)
def head_reference(case):
    """(logits, upsample64 of them, its argmax_first, its margin) - computed once per case and process, never modified"""
    x = case.logits()
    v = upsample64(x, case.ho, case.wo)
    return x, v, argmax_first(v), margin(v)
