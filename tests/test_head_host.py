"""The float64 reference of the head (tests/head_ref64.py) pinned with references alone, on the CPU, at every shape the GPU tests
(tests/test_gpu_head.py) run: fp32 ATen stays within HEAD_BAR of it, interpolation with float64 coordinates does not (the bar
bites on a coordinate error), near-ties are rare enough for the argmax comparison, and the two deliberate errors a kernel could
make - one column's tap one to the right, last maximum instead of first - are visible at the bars the GPU tests use."""
import pytest
import torch
import torch.nn.functional as F

import head_ref64 as R

ALL_CASES = R.HEAD_CASES + [c for c in R.LOSS_CASES if c.b != 2]      # (the small loss cases are head shapes, same logits)
IDS = [c.name for c in ALL_CASES]


def _um(err, x):
    return float(err) / (R.U * float(x.abs().max()))


@pytest.mark.parametrize('case', ALL_CASES, ids=IDS)
def test_fp32_aten_is_within_head_bar(case):
    x, v, _, _ = R.head_reference(case)
    aten = F.interpolate(x, size=(case.ho, case.wo), mode='bilinear', align_corners=True)
    err = float((aten.double() - v).abs().max())
    print(case.name, 'fp32 ATen: %.2f u*M' % _um(err, x))
    assert err <= R.head_bar(x), (err, R.head_bar(x))


@pytest.mark.parametrize('case', ALL_CASES, ids=IDS)
def test_float64_coordinates_are_outside_head_bar(case):
    x, v, _, _ = R.head_reference(case)
    f64 = F.interpolate(x.double(), size=(case.ho, case.wo), mode='bilinear', align_corners=True)
    err = float((f64 - v).abs().max())
    print(case.name, 'float64 coordinates: %.1f u*M = %.2e * M' % (_um(err, x), err / float(x.abs().max())))
    if case.name in R.EXACT_COORDS:
        assert err <= R.head_bar(x), (err, R.head_bar(x))      # scale 0, 1 or a power of two: nothing to round
    else:
        assert err > R.head_bar(x), (err, R.head_bar(x))


@pytest.mark.parametrize('case', ALL_CASES, ids=IDS)
def test_near_ties_are_rare(case):
    x, _, _, mg = R.head_reference(case)
    near = int((mg <= 2 * R.head_bar(x)).sum())
    print(case.name, 'near ties: %d of %d pixels' % (near, mg.numel()))
    assert near <= R.NEAR_TIE_CAP * mg.numel(), (near, mg.numel())


def test_labels_of_the_loss_cases_have_every_kind():
    for case in R.LOSS_CASES:
        lab = case.labels()
        assert bool((lab[0] == 255).all()) and bool((lab == 200).any()) and bool((lab == -1).any()) and bool((lab == -100).any())
        assert torch.equal(case.labels_u8().long(), torch.where(lab < 0, torch.full_like(lab, 255), lab))
        if case.b == 2:                                       # (the small ones: the reference of the large case is the GPU test's)
            nll, valid, correct = R.seg_loss64(case.logits(), lab, case.ho, case.wo, 255)
            assert valid == int(((lab >= 0) & (lab < case.c)).sum()) and 0 < correct < valid and nll > 0


def test_one_column_off_is_outside_head_bar():
    """the first tap of one output column read one source column to the right: far more than HEAD_BAR, in that column only"""
    case = R.HEAD_CASES[1]                                    # 18 x 75 -> 70 x 300
    x, v, _, _ = R.head_reference(case)
    col = 257                                                # the second lane of the second 256-wide column tile
    d = (R.upsample64(x, case.ho, case.wo, bump_col=col) - v).abs()
    assert float(d[..., col].max()) > 1e4 * R.head_bar(x)
    d[..., col] = 0
    assert float(d.max()) == 0.0


def test_first_maximum_wins_is_visible():
    """channel 7 a bitwise copy of channel 2: first-wins never answers 7, last-wins answers 7 wherever the pair is on top"""
    case = R.HEAD_CASES[0]
    x = case.logits()
    x[:, 7] = x[:, 2]
    v = R.upsample64(x, case.ho, case.wo)
    first, last = R.argmax_first(v), R.argmax_first(v, last=True)
    assert not bool((first == 7).any()) and bool((first == 2).any())
    assert bool((last[first == 2] == 7).all()) and torch.equal(first[first != 2], last[first != 2])
    # constant logits: label 0 everywhere
    assert not bool(R.argmax_first(torch.full((2, 5, 3, 4), 1.5, dtype=torch.float64)).any())
