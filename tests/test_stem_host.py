"""The stem's float64 checker (tests/stem_ref64.py) pinned without a GPU: the bar holds for correct fp32 arithmetic in the kernels'
order at every shape tests/test_gpu_stem.py runs, it bites (each wrong stem below exceeds it at some element by at least 10x),
stem_inputs() is the oracle's input tensor bit for bit, and the ReLU hides at most a fifth of any run's outputs."""
import pytest
import torch
import torch.nn.functional as F

import stem_ref64 as R

DU16, LUT = R.PF_HOP_DEPTH_U16, R.PF_HOP_TRAINID_LUT


def _shapes():
    """one case per (T, n_cls, H, W) of the GPU tests"""
    seen = {}
    for c in R.CASES:
        seen.setdefault((c.T, c.n_cls, c.h, c.w), c)
    return list(seen.values())


SHAPES = _shapes()


@pytest.mark.parametrize('case', SHAPES, ids=[c.name for c in SHAPES])
def test_bar_holds_for_fp32_arithmetic_in_the_kernels_order(case):
    w, b = R.params(case)
    worst = 0.0
    for hop, ps in ((0, 1), (DU16 | LUT, 0)):
        x, ref, bar = R.reference(case, hop, ps)
        got = R.emulate_fp32(x, w, b, case.T, case.n_cls).double()
        assert got.shape == ref.shape
        ratio = float(((got - ref).abs() / bar).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (hop, ps, ratio)
    print(case.name, 'emulation err / bar = %.3g' % worst)


@pytest.mark.parametrize('case', R.CASES, ids=[c.name for c in R.CASES])
def test_relu_hides_at_most_a_fifth(case):
    for hop, ps in case.runs:
        assert R.positive_share(case, hop, ps) >= 0.8, (hop, ps, R.positive_share(case, hop, ps))


def test_the_set_with_an_infinite_std_zeroes_the_depth_channels_and_meets_the_bar():
    """what tests/test_gpu_stem.py::test_ieee_division_under_the_depth_hop relies on"""
    for case in [c for c in R.V4_CASES if c.n_cls == 11]:
        w, b = R.params(case)
        for hop in (DU16, DU16 | LUT):
            x, ref, bar = R.reference(case, hop, R.INF_STD_SET)
            assert not bool(x[:, case.T * case.n_cls:].any()) and bool(torch.isfinite(x).all())
            assert R.positive_share(case, hop, R.INF_STD_SET) >= 0.8
            assert float(((R.emulate_fp32(x, w, b, case.T, case.n_cls).double() - ref).abs() / bar).max()) <= 1.0


def _case(name):
    return next(c for c in R.CASES if c.name == name)


BITE_CASES = [_case('v4 u8 T3 C11 20x264 B1'), _case('v3 i64 T3 C11 7x9 B2'), _case('generic u8 T5 C19 5x130 B1'),
              _case('generic i64 T1 C19 7x9 B2')]


def _excess(out, ref, bar):
    return float(((out - ref).abs() / bar).max())


@pytest.mark.parametrize('case', BITE_CASES, ids=[c.name for c in BITE_CASES])
def test_bar_bites(case):
    """each wrong stem, evaluated in float64 (no rounding of its own), is at least 10 bars away from the reference somewhere"""
    w, b = R.params(case)
    T, C = case.T, case.n_cls
    hop, ps = DU16, 1
    mean, std, dmin, dmax = R.PARAM_SETS[ps]
    x, ref, bar = R.reference(case, hop, ps)
    seg, depth, _ = R.planes(case, hop)
    t, ky, kx = T - 1, 2, 1
    found = {}

    w2 = w.clone()
    w2[:, t * C:(t + 1) * C, ky, kx] = 0
    found['one (tap, frame) one-hot group dropped'] = _excess(R.stem64(x, w2, b), ref, bar)
    w2 = w.clone()
    w2[:, T * C + t, ky, kx] = 0
    found['one depth tap dropped'] = _excess(R.stem64(x, w2, b), ref, bar)
    ho, wo = ref.shape[-2:]
    shifted = F.relu(F.conv2d(F.pad(x.double(), (0, 2, 0, 2)), w.double(), b.double(), stride=2))[..., :ho, :wo]
    found['window shifted by one pixel'] = _excess(shifted, ref, bar)
    seg2 = torch.where(seg.long() == C, torch.zeros_like(seg.long()), seg.long())
    assert bool((seg.long() == C).any())
    found['label n_cls taken as class 0'] = _excess(
        R.stem64(R.stem_inputs(seg2, depth, None, T, C, mean, std, hop, dmin, dmax), w, b), ref, bar)
    assert bool(((R.hop_depth(depth, 0.0, dmax)[0] > 0) & (R.hop_depth(depth, 0.0, dmax)[0] < dmin)).any())
    found['min_depth clamp skipped'] = _excess(
        R.stem64(R.stem_inputs(seg, depth, None, T, C, mean, std, hop, 0.0, dmax), w, b), ref, bar)
    # mask = d >= 0: a depth of exactly 0 behind the hop stays unmasked and is clamped to min_depth
    d, m = R.hop_depth(depth, dmin, dmax)
    q0 = torch.round((depth + 1).clamp(0, 255) * 256) == 256
    assert bool(q0.any())
    d = torch.where(q0, torch.tensor(dmin, dtype=torch.float32), d)
    x2 = R.stem_inputs(seg, d, (m | q0).to(torch.uint8), T, C, mean, std, 0, dmin, dmax)
    assert not torch.equal(x2, x)
    found['mask = d >= 0 in place of d > 0'] = _excess(R.stem64(x2, w, b), ref, bar)

    print(case.name, {k: '%.3g' % v for k, v in found.items()})
    for what, ratio in found.items():
        assert ratio >= 10.0, (what, ratio)


def test_stem_inputs_equals_the_oracles_input_tensor():
    from oracle import hardnet_ref
    case = _case('v3 i64 T3 C11 7x9 B2')
    seg, depth, mask = R.planes(case, 0)
    assert bool((seg >= 2 ** 32).any()) and bool((seg == case.n_cls).any())
    mean, std, dmin, dmax = R.PARAM_SETS[1]
    sd = {'depth_mean': torch.tensor([mean]), 'depth_std': torch.tensor([std])}
    want = hardnet_ref.bg_inputs_to_tensor(sd, seg, depth, mask, num_classes=case.n_cls)
    got = R.stem_inputs(seg, depth, mask, case.T, case.n_cls, mean, std, 0, dmin, dmax)
    assert got.dtype == want.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_hop_depth_equals_the_oracles_hop():
    """export to u16 and load (oracle/hop.py) on the edge values of both parameter sets"""
    from oracle import hop as ohop
    for _, _, dmin, dmax in R.PARAM_SETS:
        d = torch.tensor(R.depth_edges(dmin, dmax) + [3.3, 77.7, 150.2], dtype=torch.float32)
        want_d, want_m = ohop.load_depth(ohop.export_depth_u16(d), dmin, dmax)
        got_d, got_m = R.hop_depth(d, dmin, dmax)
        assert torch.equal(got_m, want_m) and torch.equal(got_d.view(torch.int32), want_d.view(torch.int32))
        assert not bool(got_m[:2].any()) and not bool(got_m[9:12].any())       # -1, the tie at code 0.5, 0, -0.0, -5: masked
        assert float(got_d[7]) == torch.tensor(dmin).item() and float(got_d[8]) == torch.tensor(dmax).item()
