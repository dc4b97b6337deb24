"""The upsample + argmax head (launch_head: head_col_kernel<11> / <19>, head4_kernel, head_kernel) and the fused validation loss
(pf_seg_loss: seg_loss_tile_kernel<11> / <19>, seg_loss_finish_kernel) one kernel at a time, against the float64 reference with
the contract's fp32 coordinates (tests/head_ref64.py; the bars HEAD_BAR = 4.5*u*M and LOSS_P are derived there, and pinned on the
CPU by tests/test_head_host.py).

The head runs behind ONE 1x1 convolution with identity weights (tests/helpers.py: MiniNet.run_head); its input is what the library
itself hands out as out_orig_logits, asserted bit-equal to the convolution's output, so the convolution's rounding is not part of
any comparison.  Per case: out_logits within HEAD_BAR of the reference elementwise; the labels equal argmax_first of the kernel's
OWN out_logits everywhere; they equal the reference's labels wherever the float64 margin exceeds 2*HEAD_BAR, and such near-ties
are at most 0.05 % of the pixels; uint8 labels, int64 labels and a run without out_logits agree; the profile names the kernel the
conditions of launch_head select (a change of those conditions must not silently empty a case); pf_last_error is untouched.  Every
case writes its worst err / (u*M), its near-tie count and its kernel to head_probe_dist.json in the suite's scratch report
directory (tests/helpers.py: head_probe_record); the run on MI355X is kept as profiles/head_probe_dist.json.

Two shapes run another kernel than a reading of the shapes alone suggests, by launch_head's own conditions: at 2x (35 x 150 ->
70 x 300) the source window of a 32 x 256 tile is 18 x 130 pixels, 103 KB at 11 classes, so the tiled head does not fit and
head_kernel runs; at 9 x 13 -> 1 x 1 with 11 classes the window is 3 x 3 and the TILED head runs (a 5-class twin reaches
head_kernel with both scales 0).  No degenerate size is refused by the library's argument checks.

To be checked once each with a deliberate wrong-value edit (values only, never an address; not kept), as tests/test_gpu_train_layers.py
was: head_col_kernel taking its second tap from the first tap's column in the second column tile; head4_kernel taking t0[1] where
i1 == 2; seg_loss_finish_kernel stopping at min(n, 256).  NOT DONE YET: this file has not run on a device; which cases fail under
each edit, and that the whole-network tests pass under them, is to be recorded here with the first MI355X run, together with
profiles/head_probe_dist.json.
"""
import ctypes
import math

import pytest
import torch

import head_ref64 as R
from helpers import MiniNet, MiniSpec, head_probe_record

pytestmark = pytest.mark.gpu

PF_EUNSUPPORTED = -5


def _net(c, weight=None, bias=None):
    from panoptic_forecasting_amd import hardnet_arch as arch
    spec = MiniSpec(c)
    spec.head(spec.conv('logit', [arch.Src(0, 0, c)], c, 1, relu=False))
    weight = torch.eye(c).view(c, c, 1, 1).contiguous() if weight is None else weight
    return MiniNet(spec, {'logit': (weight, torch.zeros(c) if bias is None else bias)})


def _head_kernels(records):
    return sorted(r['label'].replace('void ', '').replace('pf::', '').replace('(HeadArgs)', '')
                  for r in records if 'head' in r['label'] and 'HeadArgs' in r['label'])


def _forward(case, x, weight=None, bias=None):
    """the three runs of a case -> (orig, out_logits, labels, kernels that ran); asserts what holds for any input: return codes,
    pf_last_error, orig == the convolution's output bit for bit, the three label outputs identical, labels == argmax_first of
    the kernel's own out_logits"""
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    net = _net(case.c, weight, bias)
    try:
        before = L.pf_last_error()
        xg = x.cuda()
        pflib.profile(True)
        try:
            rc, seg8, logits, orig = net.run_head(xg, case.ho, case.wo, torch.uint8, True)
            records = pflib.profile_results()
        finally:
            pflib.profile(False)
        assert rc == 0, (rc, L.pf_last_error())
        conv_out = net.tensor('logit')
        rc, seg64, logits64, _ = net.run_head(xg, case.ho, case.wo, torch.int64, True)
        assert rc == 0, (rc, L.pf_last_error())
        rc, seg8n, none, _ = net.run_head(xg, case.ho, case.wo, torch.uint8, False)
        assert rc == 0 and none is None, (rc, L.pf_last_error())
        assert L.pf_last_error() == before, L.pf_last_error()
    finally:
        net.close()
    kernels = _head_kernels(records)
    assert torch.equal(orig.view(torch.int32), conv_out.view(torch.int32))            # the head's input, bit for bit
    assert torch.equal(logits.view(torch.int32), logits64.view(torch.int32))
    seg = seg8.cpu().long()
    assert torch.equal(seg, seg64.cpu()) and torch.equal(seg, seg8n.cpu().long())
    logits = logits.cpu()
    assert bool(torch.isfinite(logits).all())                                         # every element was written
    own = R.argmax_first(logits.double())
    assert int((own != seg).sum()) == 0, int((own != seg).sum())
    return orig.cpu(), logits, seg, kernels


@pytest.mark.parametrize('case', R.HEAD_CASES, ids=[c.name for c in R.HEAD_CASES])
def test_head(case):
    x, v, ref_seg, mg = R.head_reference(case)
    orig, logits, seg, kernels = _forward(case, x)
    if not torch.equal(orig, x):                 # (identity weights reproduce x exactly; if a conv kernel ever did not, the head's
        v = R.upsample64(orig, case.ho, case.wo)  # input still is `orig`)
        ref_seg, mg = R.argmax_first(v), R.margin(v)
    bar = R.head_bar(orig)
    err = float((logits.double() - v).abs().max())
    near = mg <= 2 * bar
    wrong = seg != ref_seg
    entry = {'err_uM': float('%.4g' % (err / (R.U * float(orig.abs().max())))), 'near_ties': int(near.sum()),
             'label_differs_at_near_ties': int((wrong & near).sum()), 'pixels': mg.numel(), 'kernel': kernels, 'note': case.note}
    head_probe_record(case.name, entry)
    print(case.name, entry)
    assert kernels == [case.kernel], (kernels, case.kernel)
    assert err <= bar, (err, bar)
    assert int((wrong & ~near).sum()) == 0, int((wrong & ~near).sum())
    assert int(near.sum()) <= R.NEAR_TIE_CAP * mg.numel(), (int(near.sum()), mg.numel())
    if (case.hin, case.win) == (case.ho, case.wo):           # identity: every weight is exactly 0 or 1
        assert torch.equal(logits.view(torch.int32), orig.view(torch.int32))


def _case(name):
    return next(c for c in R.HEAD_CASES if c.name == name)


# one case per kernel: (case, the channel that becomes a copy, of which lower-numbered channel)
TIES = [(_case('C11 16x80->64x320'), 7, 2), (_case('C19 18x75->70x300'), 7, 2), (_case('C11 200x13->34x40'), 7, 2),
        (_case('C5 9x13->33x40'), 4, 1), (_case('C11 64x128->32x64'), 7, 2), (_case('C5 9x13->33x41'), 4, 1)]


@pytest.mark.parametrize('case,hi,lo', TIES, ids=[c[0].name for c in TIES])
def test_first_maximum_wins(case, hi, lo):
    x = case.logits()
    x[:, hi] = x[:, lo]
    orig, logits, seg, kernels = _forward(case, x)
    assert kernels == [case.kernel], (kernels, case.kernel)
    assert torch.equal(orig[:, hi].view(torch.int32), orig[:, lo].view(torch.int32))
    assert torch.equal(logits[:, hi].view(torch.int32), logits[:, lo].view(torch.int32))
    v = R.upsample64(orig, case.ho, case.wo)
    ref_seg = R.argmax_first(v)
    clear = R.margin(v[:, [c for c in range(case.c) if c != hi]]) > 2 * R.head_bar(orig)     # the copy itself is margin 0
    assert not bool((seg == hi).any()), int((seg == hi).sum())
    assert bool((ref_seg == lo).any()) and bool((seg[(ref_seg == lo) & clear] == lo).all())


@pytest.mark.parametrize('case', [t[0] for t in TIES], ids=[c[0].name for c in TIES])
def test_constant_logits_give_label_0(case):
    x = case.logits()
    orig, logits, seg, kernels = _forward(case, x, weight=torch.zeros(case.c, case.c, 1, 1), bias=torch.full((case.c,), 1.5))
    assert kernels == [case.kernel], (kernels, case.kernel)
    assert bool((orig == 1.5).all()) and not bool(seg.any())


# ------------------------------------------------------------------------------------------------ pf_seg_loss
def _seg_loss(logits, labels, ho, wo, ignore=255):
    """-> (rc, out3 as a tuple of 3 floats, kernels recorded); out3 is pre-filled with 7.0"""
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    b, c, hin, win = logits.shape
    need = ctypes.c_size_t()
    pflib.check(L.pf_seg_loss_workspace(b, ho, wo, ctypes.byref(need)), 'pf_seg_loss_workspace')
    ws = torch.zeros(max(need.value, 256), dtype=torch.uint8, device='cuda')
    out3 = torch.full((3,), 7.0, dtype=torch.float64, device='cuda')
    lg, lb = logits.cuda().contiguous(), labels.cuda().contiguous()
    pflib.profile(True)
    try:
        rc = L.pf_seg_loss(lg.data_ptr(), b, c, hin, win, lb.data_ptr(), int(lb.dtype == torch.int64), ho, wo, ignore,
                           out3.data_ptr(), ws.data_ptr(), ws.numel(), pflib.stream_ptr())
        torch.cuda.synchronize()
        records = pflib.profile_results()
    finally:
        pflib.profile(False)
    return rc, tuple(out3.cpu().tolist()), sorted(r['label'].replace('void pf::', '').replace('(pf::LossArgs)', '') for r in records)


@pytest.mark.parametrize('case', R.LOSS_CASES, ids=[c.name for c in R.LOSS_CASES])
def test_seg_loss(case):
    """LOSS_P (tests/head_ref64.py) per valid pixel; valid exact; correct within the near-tie pixels; uint8 == int64 labels"""
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    x, v, ref_seg, mg = R.head_reference(case)
    lab = case.labels()
    assert bool((lab[0] == 255).all()) and bool((lab == 200).any()) and bool((lab < 0).any())
    nll, valid, correct = R.seg_loss64(x, lab, case.ho, case.wo, 255, v=v)
    m = float(x.abs().max())
    near = int((mg <= 2 * R.head_bar(x)).sum())
    before = L.pf_last_error()
    rc, out64, kernels = _seg_loss(x, lab, case.ho, case.wo)
    assert rc == 0, (rc, L.pf_last_error())
    rc, out8, _ = _seg_loss(x, case.labels_u8(), case.ho, case.wo)
    assert rc == 0 and L.pf_last_error() == before, (rc, L.pf_last_error())
    p = R.loss_p(m, case.c, valid)
    entry = {'nll_err_per_valid_pixel_u': float('%.4g' % (abs(out64[0] - nll) / valid / R.U)), 'bar_u': float('%.4g' % (p / R.U)),
             'valid': valid, 'correct_hip': out64[2], 'correct_ref': correct, 'near_ties': near, 'kernel': kernels,
             'partial_sums': case.b * math.ceil(case.ho / 16) * math.ceil(case.wo / 256), 'note': case.note}
    head_probe_record('loss ' + case.name, entry)
    print(case.name, entry)
    assert kernels == [case.kernel], kernels             # (the one-block finish kernel is enqueued outside the profile scope)
    assert out64 == out8, (out64, out8)
    assert out64[1] == valid, (out64[1], valid)
    assert abs(out64[2] - correct) <= near, (out64[2], correct, near)
    assert abs(out64[0] - nll) <= valid * p, (out64[0], nll, valid * p)


def test_seg_loss_with_every_label_ignored_is_zero():
    case = R.LOSS_CASES[1]
    lab = torch.full((case.b, case.ho, case.wo), 255, dtype=torch.uint8)
    rc, out3, _ = _seg_loss(case.logits(), lab, case.ho, case.wo)
    assert rc == 0 and out3 == (0.0, 0.0, 0.0), (rc, out3)


def test_seg_loss_refuses_a_window_that_does_not_fit():
    """identity ratio, 11 classes: 18 x 258 source pixels per 16 x 256 tile = 204 KB > 60 KB -> PF_EUNSUPPORTED, nothing launched"""
    from panoptic_forecasting_amd import lib as pflib
    case = _case('C11 20x30->20x30')
    rc, out3, kernels = _seg_loss(case.logits(), case.labels(), 20, 30)
    assert rc == PF_EUNSUPPORTED, rc
    assert b'LDS' in pflib.load().pf_last_error()
    assert kernels == [] and out3 == (7.0, 7.0, 7.0), (kernels, out3)
