"""The fused one-hot stem (csrc/stem_kernels.hip: launch_stem, the choice of csrc/net_select.cpp) one kernel at a time against the float64 reference of
tests/stem_ref64.py (the bar and the cases are derived there and pinned on the CPU by tests/test_stem_host.py).

The stem runs as the first op of a three-op network, stem -> fin (1x1, 16 -> n_cls, bias, no ReLU) -> head, through pf_bg_forward
(tests/helpers.py: MiniSpec.stem, MiniNet.run_bg); its output is read with pf_hardnet_tensor_read, which undoes the plan's
power-of-two channel scales exactly.  Every case runs with the four hop-flag combinations and both (mean, std, min, max) sets; per
run: status 0, |got - float64| <= bar elementwise, and the profile names the instantiation the case stands for - a change of
launch_stem's conditions must not silently move a case to another kernel.  Every case prints its worst err / bar and writes it to
stem_probe_dist.json in the suite's scratch report directory (tests/helpers.py: stem_probe_record).

Beyond the bar: the u8 (v4) and int64 (v3) runs of the same planes agree bit for bit, as do the u8 and int64 v3 variants at
10 x 6; the packed fp16-pair output the fused front end reads is the fp32 output split (hi + mid) bit for bit; the range guard
sees an overflow and a NaN in every family; arguments the stem cannot serve are refused before any launch.

int64 labels are compared with n_cls in 64 bits: the cases without the LUT carry 2^32 + 3 and 2^40, whose low 32 bits are
classes 3 and 0.

The reciprocal form of v4's division (FAST_DIV) is chosen per parameter set where launch_stem proves it exact, which holds for
both sets above; test_ieee_division_under_the_depth_hop runs the other two instantiations with a std of infinity.
"""
import math

import pytest
import torch

import stem_ref64 as R
from helpers import MiniNet, MiniSpec, stem_probe_record

pytestmark = pytest.mark.gpu

PF_EINVAL, PF_EUNSUPPORTED = -1, -5
PF_STATUS_RANGE = 1
DU16, LUT = R.PF_HOP_DEPTH_U16, R.PF_HOP_TRAINID_LUT


def _fin(g, cin, n_cls):
    return torch.randn(n_cls, cin, 1, 1, generator=g) / cin ** 0.5, torch.randn(n_cls, generator=g) * 0.1


def _stem_net(T, n_cls, w, b):
    """stem -> fin -> head"""
    from panoptic_forecasting_amd import hardnet_arch as arch
    spec = MiniSpec(T * (n_cls + 1))
    s = spec.stem('stem', T, n_cls)
    spec.head(spec.conv('fin', [arch.Src(s, 0, 16)], n_cls, 1, relu=False))
    return MiniNet(spec, {'stem': (w, b), 'fin': _fin(torch.Generator().manual_seed(3), 16, n_cls)})


def _front_net(T, n_cls, w, b):
    """stem -> 3x3 s1 16 -> 24 -> 3x3 s2 24 -> 32 -> fin -> head: the two convolutions are what conv_front.hip fuses"""
    from panoptic_forecasting_amd import hardnet_arch as arch
    g = torch.Generator().manual_seed(4)
    spec = MiniSpec(T * (n_cls + 1))
    s = spec.stem('stem', T, n_cls)
    c1 = spec.conv('c1', [arch.Src(s, 0, 16)], 24, 3)
    c2 = spec.conv('c2', [arch.Src(c1, 0, 24)], 32, 3, stride=2)
    spec.head(spec.conv('fin', [arch.Src(c2, 0, 32)], n_cls, 1, relu=False))
    P = {'stem': (w, b), 'fin': _fin(g, 32, n_cls)}
    for name, cin, cout in (('c1', 16, 24), ('c2', 24, 32)):
        P[name] = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5, torch.randn(cout, generator=g) * 0.1)
    return MiniNet(spec, P)


def _labels(records):
    return [r['label'].replace('void ', '').replace('pf::', '').split('(')[0] for r in records]


def _run(net, seg, depth, mask, hop, ps, want_rc=0):
    """one pf_bg_forward -> (stem output on the CPU or None, status, stem kernels that ran, all labels)"""
    from panoptic_forecasting_amd import lib as pflib
    mean, std, dmin, dmax = R.ALL_SETS[ps]
    ho, wo = (seg.shape[-2] + 1) // 2, (seg.shape[-1] + 1) // 2
    pflib.profile(True)
    try:
        rc = net.run_bg(seg.cuda(), depth.cuda(), None if mask is None else mask.cuda(), mean, std, hop, dmin, dmax, ho, wo)
        labels = _labels(pflib.profile_results())
    finally:
        pflib.profile(False)
    assert rc == want_rc, (rc, pflib.load().pf_last_error())
    stem = [k for k in labels if 'stem_onehot' in k]
    if rc:
        return None, None, stem, labels
    return net.tensor('stem').cpu(), net.status(), stem, labels


def _ratio(got, ref, bar):
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    return float(((got.double() - ref).abs() / bar).max())


@pytest.mark.parametrize('case', R.CASES, ids=[c.name for c in R.CASES])
def test_stem_against_float64(case):
    w, b = R.params(case)
    net = _stem_net(case.T, case.n_cls, w, b)
    worst, kernels = {}, set()
    try:
        for hop, ps in case.runs:
            seg, depth, mask = R.planes(case, hop)
            x, ref, bar = R.reference(case, hop, ps)
            got, status, stem, _ = _run(net, seg, depth, mask, hop, ps)
            assert len(stem) == 1 and stem[0] in case.kernel(hop), (hop, ps, stem, case.kernel(hop))
            assert status == 0, (hop, ps, status)
            kernels.add(stem[0])
            worst[(hop, ps)] = _ratio(got, ref, bar)
            print(case.name, 'hop %d set %d %s err / bar = %.4g status %d' % (hop, ps, stem[0], worst[(hop, ps)], status))
    finally:
        net.close()
        stem_probe_record(case.name, {'err_over_bar': {'hop%d set%d' % k: float('%.4g' % v) for k, v in worst.items()},
                                      'kernels': sorted(kernels), 'note': case.note})
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


TWINS = R.V4_CASES + [c for c in R.V3_U8_CASES if (c.h, c.w) == (10, 6)]


@pytest.mark.parametrize('case', TWINS, ids=[c.name for c in TWINS])
def test_u8_and_int64_labels_give_the_same_bits(case):
    """labels 0..255 as uint8 (v4; v3 at 10 x 6) and as int64 (v3): torch.equal stem outputs in every run"""
    w, b = R.params(case)
    net = _stem_net(case.T, case.n_cls, w, b)
    tf = lambda v: 'true' if v else 'false'
    try:
        for hop, ps in case.runs:
            seg, depth, mask = R.planes(case, hop)
            assert seg.dtype == torch.uint8
            got8, st8, k8, _ = _run(net, seg, depth, mask, hop, ps)
            got64, st64, k64, _ = _run(net, seg.long(), depth, mask, hop, ps)
            assert len(k8) == 1 and k8[0] in case.kernel(hop), (k8, case.kernel(hop))
            assert k64 == ['stem_onehot_v3_kernel<3, true, %s, %s>' % (tf(hop & DU16), tf(hop & LUT))], k64
            assert st8 == 0 and st64 == 0
            assert torch.equal(got8.view(torch.int32), got64.view(torch.int32)), (hop, ps, float((got8 - got64).abs().max()))
    finally:
        net.close()


IEEE = [c for c in R.V4_CASES if c.n_cls == 11]


@pytest.mark.parametrize('case', IEEE, ids=[c.name for c in IEEE])
def test_ieee_division_under_the_depth_hop(case):
    """stem_onehot_v4_kernel<3, true, ., false>: launch_stem takes the reciprocal form only where its proof of exactness passes,
    and that proof refuses a std that is not finite (no finite std was found for which it fails short of overflowing the
    quotient).  With std = inf every normalised depth is +-0, as in the reference's fp32 division: the bar, the status and the
    bits of the int64 (v3) run hold as for the other sets"""
    w, b = R.params(case)
    ps = R.INF_STD_SET
    net = _stem_net(case.T, case.n_cls, w, b)
    tf = lambda v: 'true' if v else 'false'
    try:
        for hop in (DU16, DU16 | LUT):
            seg, depth, _ = R.planes(case, hop)
            x, ref, bar = R.reference(case, hop, ps)
            got, status, stem, _ = _run(net, seg, depth, None, hop, ps)
            assert stem == ['stem_onehot_v4_kernel<3, true, %s, false>' % tf(hop & LUT)], stem
            assert status == 0
            ratio = _ratio(got, ref, bar)
            print(case.name, 'hop %d std inf %s err / bar = %.4g' % (hop, stem[0], ratio))
            assert ratio <= 1.0, ratio
            got64, st64, k64, _ = _run(net, seg.long(), depth, None, hop, ps)
            assert k64 == ['stem_onehot_v3_kernel<3, true, true, %s>' % tf(hop & LUT)] and st64 == 0, (k64, st64)
            assert torch.equal(got.view(torch.int32), got64.view(torch.int32))
    finally:
        net.close()


@pytest.fixture
def raw_ranges():
    """plans created without the per-channel power-of-two scaling: stored values are the network's own"""
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    pflib.check(L.pf_set_option(b'normalize_ranges', 0), 'pf_set_option')
    yield
    pflib.check(L.pf_set_option(b'normalize_ranges', 1), 'pf_set_option')


def _case(name):
    return next(c for c in R.CASES if c.name == name)


PACKED = [_case('v4 u8 T3 C11 16x256 B2'), _case('v4 u8 T3 C11 20x264 B1')]


@pytest.mark.parametrize('normalize', [1, 0], ids=['default plan', 'raw ranges'])
@pytest.mark.parametrize('case', PACKED, ids=[c.name for c in PACKED])
def test_packed_output_is_the_fp32_output_split(case, normalize):
    """the default plan fuses the two convolutions behind the stem (conv_front) and the stem writes fp16 pairs; read back (hi +
    mid) they equal the split of the fp32 output of the same plan spec with fuse_front = 0, bit for bit.  The split is taken of
    the value as STORED: the default plan stores a channel times a power of two s (stored_tensor() of the fp32 run), and
    pf_hardnet_tensor_read multiplies hi + mid by 1 / s; with raw ranges (normalize_ranges = 0) s = 1"""
    from panoptic_forecasting_amd import lib as pflib
    w, b = R.params(case)
    pflib.check(pflib.load().pf_set_option(b'normalize_ranges', normalize), 'pf_set_option')
    try:
        packed, plain = _front_net(case.T, case.n_cls, w, b), _front_net(case.T, case.n_cls, w, b).set_option('fuse_front', 0)
    finally:
        pflib.check(pflib.load().pf_set_option(b'normalize_ranges', 1), 'pf_set_option')
    try:
        for hop, ps in case.runs:
            seg, depth, mask = R.planes(case, hop)
            x, ref, bar = R.reference(case, hop, ps)
            gp, sp, kp, lp = _run(packed, seg, depth, mask, hop, ps)
            gf, sf, kf, lf = _run(plain, seg, depth, mask, hop, ps)
            stored = plain.stored_tensor('stem').cpu()
            assert any('conv_front' in k for k in lp) and not any('conv_front' in k for k in lf), (lp, lf)
            assert len(kp) == 1 and kp == kf and kp[0] in case.kernel(hop), (kp, kf)
            assert sp == 0 and sf == 0
            assert _ratio(gf, ref, bar) <= 1.0
            inv_s = torch.ones(16)
            for c in range(16):
                nz = stored[:, c] != 0
                r = (gf[:, c][nz] / stored[:, c][nz]).unique()
                assert len(r) == 1 and math.frexp(float(r[0]))[0] == 0.5, (c, r)             # one power of two per channel
                inv_s[c] = r[0]
            assert normalize or bool((inv_s == 1).all())
            hi = stored.half()
            mid = (stored - hi.float()).half()
            want = (hi.float() + mid.float()) * inv_s.view(1, 16, 1, 1)
            assert torch.equal(gp.view(torch.int32), want.view(torch.int32)), (hop, ps, float((gp - want).abs().max()))
    finally:
        packed.close()
        plain.close()


# one case per family: v4, v3 with int64 and with u8 labels, generic with u8 and with int64 labels
GUARDED = [_case('v4 u8 T3 C11 4x4 B1'), _case('v4 u8 T3 C19 20x264 B1'), _case('v3 i64 T3 C11 7x9 B2'), _case('v3 u8 T3 C11 7x9 B1'),
           _case('generic u8 T2 C3 7x9 B2'), _case('generic i64 T4 C11 7x9 B2')]


@pytest.mark.parametrize('case', GUARDED, ids=[c.name for c in GUARDED])
def test_an_output_above_65504_raises_the_range_flag(case, raw_ranges):
    """weights and bias times 2 * 65504 / max(reference): the largest stored output is 131008; unscaled, the status stays 0"""
    w, b = R.params(case)
    hop, ps = 0, 0
    seg, depth, mask = R.planes(case, hop)
    x, ref, bar = R.reference(case, hop, ps)
    k = 2 * 65504.0 / float(ref.max())
    for scale, flag in ((1.0, 0), (k, PF_STATUS_RANGE)):
        net = _stem_net(case.T, case.n_cls, w * scale, b * scale)
        try:
            got, status, stem, _ = _run(net, seg, depth, mask, hop, ps)
        finally:
            net.close()
        assert len(stem) == 1 and stem[0] in case.kernel(hop), stem
        assert status & PF_STATUS_RANGE == flag, (scale, status)
        assert float(got.max()) > 65504 if flag else status == 0


@pytest.mark.parametrize('case', GUARDED, ids=[c.name for c in GUARDED])
def test_a_nan_depth_is_flagged_unless_the_hop_absorbs_it(case):
    """NaN depth under a zero mask: NaN * 0 is NaN in the reference's fp32 conv, and the ReLU's max would drop it: the kernels raise
    PF_STATUS_RANGE.  Under PF_HOP_DEPTH_U16 the clamp turns NaN + 1 into code 0 (depth -1, masked): no flag, and the output
    meets the bar computed with -1 in its place"""
    w, b = R.params(case)
    seg, depth, mask = R.planes(case, 0)
    at = (case.b - 1, case.T - 1, case.h // 2, case.w // 2)
    depth, mask = depth.clone(), mask.clone()
    depth[at], mask[at] = float('nan'), 0
    net = _stem_net(case.T, case.n_cls, w, b)
    try:
        got, status, stem, _ = _run(net, seg, depth, mask, 0, 0)
        assert len(stem) == 1 and stem[0] in case.kernel(0), stem
        assert status & PF_STATUS_RANGE, status
        got, status, stem, _ = _run(net, seg, depth, None, DU16, 0)
        assert len(stem) == 1 and stem[0] in case.kernel(DU16), stem
    finally:
        net.close()
    assert status == 0, status
    depth[at] = -1.0
    mean, std, dmin, dmax = R.PARAM_SETS[0]
    x = R.stem_inputs(seg, depth, None, case.T, case.n_cls, mean, std, DU16, dmin, dmax)
    assert _ratio(got, R.stem64(x, w, b), R.stem_bar(x, w, b, case.T)) <= 1.0


# ------------------------------------------------------------------------------------------------ refusals: return codes, no launch
def _planes(b, t, h, w, dtype=torch.uint8):
    return torch.zeros(b, t, h, w, dtype=dtype), torch.ones(b, t, h, w), torch.ones(b, t, h, w, dtype=torch.uint8)


def test_weights_beyond_the_lds_budget_are_refused():
    """T * (n_cls + 1) = 105 > 104 rows of 9 * 16 floats"""
    T, n_cls = 5, 20
    net = _stem_net(T, n_cls, torch.zeros(16, T * (n_cls + 1), 3, 3), torch.zeros(16))
    try:
        _, _, stem, _ = _run(net, *_planes(1, T, 7, 9), 0, 0, want_rc=PF_EUNSUPPORTED)
    finally:
        net.close()
    assert stem == []


def test_a_frame_count_other_than_the_plans_is_refused():
    net = _stem_net(3, 11, torch.zeros(16, 36, 3, 3), torch.zeros(16))
    try:
        _, _, stem, _ = _run(net, *_planes(1, 2, 8, 8), 0, 0, want_rc=PF_EUNSUPPORTED)
    finally:
        net.close()
    assert stem == []


def test_a_missing_mask_without_the_depth_hop_is_refused():
    net = _stem_net(3, 11, torch.zeros(16, 36, 3, 3), torch.zeros(16))
    try:
        seg, depth, _ = _planes(1, 3, 8, 8)
        _, _, stem, labels = _run(net, seg, depth, None, LUT, 0, want_rc=PF_EINVAL)
    finally:
        net.close()
    assert labels == []
