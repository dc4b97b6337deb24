"""Which kernel a stem, head or validation-loss launch runs (no GPU): csrc/net_select.cpp through pf_debug_net_choice.  The GPU tests
(test_gpu_stem.py, test_gpu_head.py) see the choice only as the profile label of a launch; here the label, grid, workgroup size and LDS
bytes of every case of tests/stem_ref64.py and tests/head_ref64.py are compared with what the cases say and with a restatement of the
geometry, the refusals are provoked, and the host proof behind v4's reciprocal division (FAST_DIV) is checked against an evaluation of
all 65 281 codes that does not go through the library."""
import ctypes
import json
import os

import numpy as np
import pytest

import head_ref64 as H
import stem_ref64 as R
from conftest import GOLDEN
from panoptic_forecasting_amd import lib as pflib

PF_EUNSUPPORTED = -5
GENERIC, V3, V4 = 0, 1, 2
SEG64, HOP_D, HOP_LUT, FAST_DIV = 1, 2, 4, 8
DU16 = R.PF_HOP_DEPTH_U16


def choice(what, iargs, fargs=()):
    """(rc, label without 'void ', 'pf::' and the argument list, out[8]) of pf_debug_net_choice"""
    ia = (ctypes.c_int * len(iargs))(*iargs)
    fa = (ctypes.c_float * max(1, len(fargs)))(*fargs)
    label = ctypes.create_string_buffer(128)
    out = (ctypes.c_longlong * 8)()
    rc = pflib.load().pf_debug_net_choice(what, ia, len(iargs), fa if fargs else None, len(fargs), label, 128, out, 8)
    return rc, label.value.decode().replace('void ', '').replace('pf::', '').split('(')[0], list(out)


def stem(T, n_cls, h, w, b=1, i64=False, hop=0, dst_fmt=0, packed=True, params=R.PARAM_SETS[0]):
    return choice(0, [T, n_cls, h, w, (h + 1) // 2, (w + 1) // 2, b, int(i64), hop, dst_fmt, int(packed)], params)


def head(c):
    return choice(1, [c.b, c.c, c.hin, c.win, c.ho, c.wo])


def loss(c, ho=None, wo=None):
    return choice(2, [c.b, c.c, c.hin, c.win, ho or c.ho, wo or c.wo])


def ceil_div(a, b):
    return -(-a // b)


# ---- the stem

@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_stem_cases_run_the_kernel_they_stand_for(case):
    ho, wo = (case.h + 1) // 2, (case.w + 1) // 2
    for hop, ps in case.runs:
        rc, label, out = stem(case.T, case.n_cls, case.h, case.w, case.b, case.i64, hop, params=R.PARAM_SETS[ps])
        assert rc == 0 and label in case.kernel(hop), (hop, ps, rc, label)
        family = {'generic': GENERIC, 'v3': V3, 'v4': V4}[case.family]
        # 256 lanes: 64 x 4 outputs per workgroup, 128 x 8 for v4 (2 x 2 per lane); LDS: 9 taps x T x (n_cls + 1) rows of 16 floats
        tw, th = (128, 8) if family == V4 else (64, 4)
        assert out[:6] == [family, ceil_div(wo, tw), ceil_div(ho, th), case.b, 256, 9 * case.T * (case.n_cls + 1) * 16 * 4], (hop, ps, out)
        flags = out[6]
        assert bool(flags & HOP_D) == bool(hop & DU16) and bool(flags & HOP_LUT) == bool(hop & R.PF_HOP_TRAINID_LUT)
        assert bool(flags & SEG64) == case.i64
        # the reciprocal division: never outside v4 or without the depth hop; for both parameter sets wherever it can be
        assert bool(flags & FAST_DIV) == (family == V4 and bool(hop & DU16)), (hop, ps, flags)
        assert label.endswith('true>') == bool(flags & FAST_DIV) or family != V4


def test_stem_without_the_repacked_weights_or_past_32_bit_offsets_is_generic():
    assert stem(3, 11, 16, 256)[1].startswith('stem_onehot_v4_kernel')
    assert stem(3, 11, 16, 256, packed=False)[1] == 'stem_onehot_kernel'
    assert stem(3, 11, 1 << 16, 1 << 15)[1] == 'stem_onehot_kernel'            # T * H * W = 3 * 2^31 >= 2^32
    assert stem(3, 11, 1 << 15, 1 << 15)[1].startswith('stem_onehot_v4_kernel')


def test_stem_refusals():
    L = pflib.load()
    assert 9 * 3 * 35 * 16 * 4 > 60000 >= 9 * 3 * 34 * 16 * 4
    assert stem(3, 33, 16, 256)[0] == 0
    assert stem(3, 34, 16, 256)[0] == PF_EUNSUPPORTED and b'LDS budget' in L.pf_last_error()
    assert stem(3, 11, 16, 256, dst_fmt=1)[0] == 0                              # v4 writes the packed pairs
    for kw in (dict(h=10, w=6), dict(h=20, w=264, i64=True), dict(h=20, w=264, T=4), dict(h=20, w=264, packed=False)):
        a = dict(T=3, n_cls=11, dst_fmt=1)
        a.update(kw)
        assert stem(**a)[0] == PF_EUNSUPPORTED and b'fp32 only' in L.pf_last_error(), kw


def f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32)


def fast_div_exact_ref(mean, std, dmin, dmax):
    """The proof of stem_fast_div_exact without the library: for the 65 281 codes c of the depth hop, x = clamp(c / 256 - 1) - mean,
    is q0 = x * r, q1 = fma(fma(-q0, std, x), r, q0) with r = 1 / std, every step rounded to fp32, bit for bit the fp32 quotient x / std?
    float64 holds a sum, product or quotient of two fp32 numbers closely enough that rounding it again to fp32 gives the correctly
    rounded fp32 result (53 >= 2 * 24 + 2 bits); a fused multiply-add has no such guarantee, so its float64 sum is first rounded to odd
    (TwoSum gives the error's sign), after which the second rounding is the correct one."""
    mean, std, dmin, dmax = (np.float32(v) for v in (mean, std, dmin, dmax))
    if not np.isfinite(std) or std == 0:
        return False

    def fma32(a, b, c):                                       # fp32 fma(a, b, c): a * b is exact in float64
        p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        odd = (s.view(np.int64) & 1) == 1
        fix = np.isfinite(s) & (err != 0) & ~odd
        toward = np.where((err > 0) == (s > 0), 1, -1)         # one unit in the last place towards the exact value
        s = np.where(fix, (s.view(np.int64) + toward).view(np.float64), s)
        return s.astype(np.float32)

    with np.errstate(all='ignore'):
        d = f32(np.arange(65281, dtype=np.float64) / 256.0 - 1.0)                       # exact in fp32
        d = np.where(d > 0, np.minimum(np.maximum(d, dmin), dmax), np.float32(-1.0)).astype(np.float32)
        x = f32(d.astype(np.float64) - np.float64(mean))
        r = f32(np.float64(1.0) / np.float64(std))
        stdv = np.full_like(x, std)
        q0 = f32(x.astype(np.float64) * np.float64(r))
        q1 = fma32(fma32(-q0, stdv, x), np.full_like(x, r), q0)
        want = f32(x.astype(np.float64) / np.float64(std))
    return bool(np.array_equal(q1.view(np.uint32), want.view(np.uint32)))


FAST_DIV_SETS = R.ALL_SETS + ((20.0, 1e-38, 0.1, 200.0), (0.0, 1.0, 0.1, 200.0), (3.25, 0.37, 1.0, 90.0), (20.0, -15.0, 0.1, 200.0),
                              (20.0, 0.0, 0.1, 200.0), (1e30, 3.0, 0.1, 200.0), (20.0, 3e38, 0.1, 200.0))


@pytest.mark.parametrize('params', FAST_DIV_SETS, ids=lambda p: 'mean%g-std%g-%g-%g' % p)
def test_fast_div_is_chosen_where_it_is_exact_on_all_65281_codes(params):
    want = fast_div_exact_ref(*params)
    if params in R.PARAM_SETS:
        assert want
    if params == R.ALL_SETS[R.INF_STD_SET] or params[1] == 1e-38:                      # 235 / 1e-38 overflows: q0 = inf, q1 = NaN
        assert not want
    for hop in R.HOPS:
        rc, label, out = stem(3, 11, 16, 256, hop=hop, params=params)
        assert rc == 0 and bool(out[6] & FAST_DIV) == (want and bool(hop & DU16)), (hop, label, out)
        assert label.startswith('stem_onehot_v4_kernel') and label.endswith('true>' if out[6] & FAST_DIV else 'false>')
    assert not stem(3, 11, 10, 6, hop=DU16, params=params)[2][6] & FAST_DIV            # v3


# ---- the head and the loss

@pytest.mark.parametrize('case', H.HEAD_CASES, ids=lambda c: c.name + ' ' + c.kernel)
def test_head_cases_run_the_kernel_they_stand_for(case):
    rc, label, out = head(case)
    assert rc == 0 and label == case.kernel, (label, out)
    if label.startswith('head_col_kernel'):                  # one lane per column of a 32 x 256 tile; the staged window fits
        assert out[:5] == [2, ceil_div(case.wo, 256), ceil_div(case.ho, 32), case.b, 256] and 0 < out[5] <= 60 * 1024 and out[6] == case.c
        assert out[5] % (4 * case.c) == 0
    else:                                                    # grid-stride kernels, no dynamic LDS
        items = case.b * case.ho * (case.wo // 4 if label == 'head4_kernel' else case.wo)
        assert out[:6] == [int(label == 'head4_kernel'), min(4096, max(1, ceil_div(items, 256))), 1, 1, 256, 0]


@pytest.mark.parametrize('case', H.LOSS_CASES, ids=lambda c: '%s B%d' % (c.name, c.b))
def test_loss_cases_and_the_workspace(case):
    rc, label, out = loss(case)
    assert rc == 0 and label == case.kernel
    blocks = case.b * ceil_div(case.ho, 16) * ceil_div(case.wo, 256)
    assert out[1:5] == [ceil_div(case.wo, 256), ceil_div(case.ho, 16), case.b, 256] and out[6] == blocks and 0 < out[5] <= 60 * 1024
    need = ctypes.c_size_t()
    assert pflib.load().pf_seg_loss_workspace(case.b, case.ho, case.wo, ctypes.byref(need)) == 0
    assert need.value == out[7] == ceil_div(blocks * 24, 256) * 256


def test_loss_refusals():
    L = pflib.load()
    case = next(c for c in H.HEAD_CASES if c.name == 'C11 20x30->20x30')     # test_seg_loss_refuses_a_window_that_does_not_fit
    assert loss(case)[0] == PF_EUNSUPPORTED and b'LDS' in L.pf_last_error()   # 18 x 258 source pixels x 11 classes = 204 KB
    for c in (5, 12, 0):
        assert choice(2, [2, c, 16, 80, 64, 320])[0] == PF_EUNSUPPORTED and b'11 or 19 classes' in L.pf_last_error()
    assert choice(2, [2, 11, 16, 80, 64, 320])[0] == 0


# ---- the schedule and the selector agree on v4

def test_the_schedule_fuses_the_front_end_exactly_where_the_selector_says_v4():
    """(tests/test_hardnet_schedule_host.py asserts S_STEM_FRONT for 4-aligned sizes only; the other side is here)"""
    from panoptic_forecasting_amd import packing, synth
    from test_hardnet_schedule_host import KIND, S, schedule
    with open(os.path.join(GOLDEN, 'calib_seed1234.json')) as f:
        blob = packing.pack_blob(synth.make_state_dict(seed=1234, calib=json.load(f)), 36, 11)
    for h, w in ((64, 128), (64, 130), (66, 128)):
        _, rows = schedule(blob, 36, 11, 2, h, w, h, w, 3)
        v4 = stem(3, 11, h, w, 2, hop=DU16)[2][0] == V4
        assert v4 == (h % 4 == 0 and w % 4 == 0)
        assert rows[0, KIND] == (S['S_STEM_FRONT'] if v4 else S['S_STEM']), (h, w)
