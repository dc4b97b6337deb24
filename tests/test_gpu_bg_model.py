"""HIP bg network (pf_bg_forward through BGModel) vs the reference fixtures (g3) and the torch oracle.

Tolerances (stated by the parity contract): fp32 path, logits of O(1):
  max |orig_size_logits - ref| <= 1e-3,  argmax agreement >= 99.9 %.
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), 'golden')
LOGIT_TOL = 1e-3
AGREE = 0.999


def _sd():
    from panoptic_forecasting_amd import synth
    with open(os.path.join(G, 'calib_seed1234.json')) as f:
        return synth.make_state_dict(seed=1234, calib=json.load(f))


def _model(h=None, w=None, **kw):
    from panoptic_forecasting_amd.registry import build_model
    params = {'task': 'bg', 'no_gpu': False, 'load_model': None, 'load_best_model': False,
              'data': {'num_classes': 11, 'depth_norm_params': [torch.tensor([20.]), torch.tensor([15.])],
                       'min_depth': 0.1, 'max_depth': 200},
              'model': {'num_inputs': 3, 'use_depth_inps': True, 'convert2onehot': True}}
    if h is not None:
        params['model'].update(final_h=h, final_w=w)
    params['model'].update(kw)
    m = build_model(params)
    m.load_state_dict(_sd())
    m.eval()
    return m


@pytest.mark.parametrize('size', ['64x128', '96x160'])
def test_matches_reference_fixture(size):
    z = np.load(os.path.join(G, 'g3_%s.npz' % size))
    h, w = z['seg_in'].shape[-2:]
    m = _model(h, w)
    inputs = {'seg': torch.from_numpy(z['seg_in']).long().cuda(), 'depth': torch.from_numpy(z['depth']).cuda(),
              'depth_mask': torch.from_numpy(z['mask']).cuda()}
    out = m.predict(inputs, None)
    assert out['seg'].dtype == torch.int64 and out['logits'].shape == z['logits'].shape
    e1 = np.abs(out['orig_size_logits'].cpu().numpy() - z['orig_size_logits']).max()
    e2 = np.abs(out['logits'].cpu().numpy() - z['logits']).max()
    agree = (out['seg'].cpu().numpy() == z['seg']).mean()
    assert e1 <= LOGIT_TOL and e2 <= LOGIT_TOL, (e1, e2)
    assert agree >= AGREE, agree


def test_stage_by_stage_vs_oracle():
    """Every block output inside the workspace against the oracle's taps (bisecting aid)."""
    from helpers import view_tensor
    from oracle import hardnet_ref
    from panoptic_forecasting_amd import synth
    h, w = 128, 192
    m = _model(h, w)
    inp = synth.make_bg_inputs(b=1, h=h, w=w, seed=9)
    taps = {}
    ref = hardnet_ref.bg_predict(_sd(), inp, final_size=(h, w), taps=taps)
    out = m.predict({k: v.cuda() for k, v in inp.items()}, None)
    names = {'base.0': 'base.0', 'base.1': 'base.1', 'base.2': 'base.2', 'base.3': 'base.3',
             'base.4': 'base.4.out', 'base.7': 'base.7.out', 'base.10': 'base.10.out', 'base.13': 'base.13.out',
             'base.16': 'base.16.out', 'denseBlocksUp.0': 'denseBlocksUp.0.out',
             'denseBlocksUp.3': 'denseBlocksUp.3.out'}
    for tap, tname in names.items():
        got = view_tensor(m._get_plan(), m._ws, tname, 1, h, w).cpu()
        err = (got - taps[tap]).abs().max().item()
        assert err <= 1e-4 * (1 + taps[tap].abs().max().item()), (tap, err)
    assert (out['orig_size_logits'].cpu() - ref['orig_size_logits']).abs().max() <= LOGIT_TOL


# (204, 96, 3): one partial strip (24 of 31 columns), an odd number of output rows (51: the last step stores one row), 3 frames;
# (72, 264): 3 strips, 18 rows; (256, 512): segments of unequal length.  (An odd number of stem rows never reaches the kernel: the stem
# variant that writes packed pairs handles 2 x 2 outputs per lane and is only chosen for even sizes.)
@pytest.mark.parametrize('h,w,b', [(128, 192, 1), (96, 160, 2), (256, 512, 1), (72, 264, 1), (204, 96, 3)])
def test_fused_front_end_vs_oracle(h, w, b):
    """conv_front.hip: base.1 + base.2 as one kernel on the packed-pair stem output (u8 labels select the stem variant that
    writes it).  The stem output and base.2 against the oracle's taps, the logits against the oracle, and against the same
    network with the fusion switched off (three separate kernels): the fused path must actually have run."""
    from helpers import view_tensor
    from oracle import hardnet_ref
    from panoptic_forecasting_amd import lib as pflib
    from panoptic_forecasting_amd import synth
    inp = synth.make_bg_inputs(b=b, h=h, w=w, seed=h + w)
    taps = {}
    ref = hardnet_ref.bg_predict(_sd(), inp, final_size=(h, w), taps=taps)
    cu = {k: v.cuda() for k, v in inp.items()}
    cu['seg'] = cu['seg'].to(torch.uint8)                 # 255 = void stays 255
    outs = {}
    for fuse in (1, 0):        # 1: conv_front.hip; 0: three kernels
        m = _model(h, w, fuse_front=fuse)
        pflib.profile(True)
        outs[fuse] = m.predict(cu, None)
        labels = [r['label'] for r in pflib.profile_results()]
        pflib.profile(False)
        assert any('conv_front_' in l for l in labels) == bool(fuse), labels
        for tap in ('base.0', 'base.2'):
            got = view_tensor(m._get_plan(), m._ws, tap, b, h, w).cpu()
            err = (got - taps[tap]).abs().max().item()
            assert err <= 1e-4 * (1 + taps[tap].abs().max().item()), (fuse, tap, err)
        # the tensor between the two fused convs is never stored: a tap of it must fail loudly, not return workspace bytes
        if fuse:
            with pytest.raises(pflib.PfError, match='elided'):
                view_tensor(m._get_plan(), m._ws, 'base.1', b, h, w)
        else:
            got = view_tensor(m._get_plan(), m._ws, 'base.1', b, h, w).cpu()
            assert (got - taps['base.1']).abs().max().item() <= 1e-4 * (1 + taps['base.1'].abs().max().item())
        assert m.range_status() == 0
        assert (outs[fuse]['orig_size_logits'].cpu() - ref['orig_size_logits']).abs().max() <= LOGIT_TOL
        assert (outs[fuse]['seg'].cpu() == ref['seg']).float().mean().item() >= AGREE
    for fuse in (1,):
        assert (outs[fuse]['orig_size_logits'] - outs[0]['orig_size_logits']).abs().max().item() <= 1e-4


@pytest.mark.parametrize('h,w,b', [(256, 512, 1), (160, 224, 2)])
def test_matches_oracle(h, w, b):
    from oracle import hardnet_ref
    from panoptic_forecasting_amd import synth
    m = _model(h, w)
    inp = synth.make_bg_inputs(b=b, h=h, w=w, seed=2)
    ref = hardnet_ref.bg_predict(_sd(), inp, final_size=(h, w))
    out = m.predict({k: v.cuda() for k, v in inp.items()}, None)
    err = (out['orig_size_logits'].cpu() - ref['orig_size_logits']).abs().max().item()
    agree = (out['seg'].cpu() == ref['seg']).float().mean().item()
    assert err <= LOGIT_TOL, err
    assert agree >= AGREE, agree
    hist = torch.bincount(out['seg'].flatten().cpu(), minlength=11)
    assert (hist > 0).sum() >= 5          # the synthetic net must not collapse to one class


def test_u8_in_u8_out_and_no_logits():
    from panoptic_forecasting_amd import synth
    m = _model(64, 128, return_logits=False)
    inp = {k: v.cuda() for k, v in synth.make_bg_inputs(b=1, h=64, w=128, seed=4).items()}
    a = m.predict(inp, None)
    assert 'logits' not in a
    seg8, _, _ = m.run(inp['seg'].to(torch.uint8), inp['depth'], inp['depth_mask'], want_logits=False,
                       want_orig=False, seg_dtype=torch.uint8)
    assert torch.equal(seg8.long(), a['seg'])


def test_dense_path_equals_fused_path():
    """convert2onehot=False configuration (bg_model.py:61-71) through pf_hardnet_forward_dense."""
    from oracle import hardnet_ref
    from panoptic_forecasting_amd import synth
    h, w = 64, 96
    sd = _sd()
    inp = synth.make_bg_inputs(b=2, h=h, w=w, seed=6)
    fused = _model(h, w).predict({k: v.cuda() for k, v in inp.items()}, None)
    dense_m = _model(h, w, convert2onehot=False)
    x = hardnet_ref.bg_inputs_to_tensor(sd, inp['seg'], inp['depth'], inp['depth_mask'])
    onehot = x[:, :33].reshape(2, 3, 11, h, w).cuda()
    d = dense_m.predict({'seg': onehot, 'depth': inp['depth'].cuda(), 'depth_mask': inp['depth_mask'].cuda()}, None)
    assert (d['orig_size_logits'] - fused['orig_size_logits']).abs().max() <= 1e-4
    assert (d['seg'] == fused['seg']).float().mean() >= AGREE


def test_dense_input_kernel_equals_the_references_arithmetic():
    """pf_bg_dense_input = bg_model.py:53-69 (one-hot with labels >= n_cls -> zero vector, the reshape of dense frames, the
    normalised + masked depth channels with an IEEE division): bit-exact against the oracle's torch restatement for u8 and i64
    labels, for dense float frames, and without depth channels."""
    import ctypes
    from oracle import hardnet_ref
    from panoptic_forecasting_amd import lib as pflib, synth
    L = pflib.load()
    h, w, b, t, n = 24, 40, 2, 3, 11
    sd = _sd()
    inp = synth.make_bg_inputs(b=b, h=h, w=w, seed=9)
    seg = inp['seg'].clone()
    seg[0, 1, :3, :5] = 255                                  # ignore labels -> zero vectors
    want = hardnet_ref.bg_inputs_to_tensor(sd, seg, inp['depth'], inp['depth_mask'])      # [B, T * (n + 1), H, W]
    mean, std = float(sd['depth_mean']), float(sd['depth_std'])
    dep, msk = inp['depth'].cuda().contiguous(), inp['depth_mask'].cuda().view(torch.uint8).contiguous()

    def run(frames, kind, c, with_depth):
        x = torch.full((b, t * c + (t if with_depth else 0), h, w), float('nan'), device='cuda')
        pflib.check(L.pf_bg_dense_input(frames.data_ptr(), kind, c, dep.data_ptr() if with_depth else None,
                                        msk.data_ptr() if with_depth else None, mean, std, b, t, h, w, x.data_ptr(), pflib.stream_ptr()),
                    'pf_bg_dense_input')
        return x.cpu()
    for frames, kind in ((seg.to(torch.uint8).cuda(), 0), (seg.long().cuda(), 1)):
        assert torch.equal(run(frames, kind, n, True).view(torch.int32), want.view(torch.int32))
        assert torch.equal(run(frames, kind, n, False), want[:, :t * n])
    dense = want[:, :t * n].reshape(b, t, n, h, w).cuda().contiguous()
    assert torch.equal(run(dense, 2, n, True).view(torch.int32), want.view(torch.int32))
    x = torch.empty(1, device='cuda')
    assert L.pf_bg_dense_input(dense.data_ptr(), 3, n, None, None, 0.0, 1.0, b, t, h, w, x.data_ptr(), pflib.stream_ptr()) == -1   # PF_EINVAL


def test_cpu_inputs_fail_loudly():
    from panoptic_forecasting_amd import synth
    from panoptic_forecasting_amd.lib import PfError
    m = _model(64, 128)
    with pytest.raises(PfError):
        m.predict(synth.make_bg_inputs(b=1, h=64, w=128), None)


@pytest.mark.parametrize('opts', [dict(fuse_pool=0, fuse_upsample=0), dict(fuse_pool=1, fuse_upsample=1)],
                         ids=['unfused', 'all_fused'])
def test_execution_options_do_not_change_the_result(opts):
    """pf_set_option: the fused epilogue stages (pool; commuted upsample) vs the oracle, same tolerance."""
    from oracle import hardnet_ref
    from panoptic_forecasting_amd import lib as pflib
    from panoptic_forecasting_amd import synth
    L = pflib.load()
    h, w = 128, 256
    try:
        for k, v in opts.items():
            pflib.check(L.pf_set_option(k.encode(), v), 'pf_set_option')
        m = _model(h, w)
        inp = synth.make_bg_inputs(b=2, h=h, w=w, seed=21)
        ref = hardnet_ref.bg_predict(_sd(), inp, final_size=(h, w))
        # a successful forward leaves pf_last_error alone (no kernel is tried and then replaced by another one)
        assert L.pf_set_option(b'no_such_option', 1) == -1
        before = L.pf_last_error()
        out = m.predict({k: v.cuda() for k, v in inp.items()}, None)
        assert L.pf_last_error() == before, L.pf_last_error()
        assert (out['orig_size_logits'].cpu() - ref['orig_size_logits']).abs().max() <= LOGIT_TOL
        assert (out['seg'].cpu() == ref['seg']).float().mean() >= AGREE
    finally:
        L.pf_set_option(b'fuse_pool', 1)
        L.pf_set_option(b'fuse_upsample', 1)
    assert L.pf_set_option(b'no_such_option', 1) == -1


@pytest.mark.parametrize('h,w,b', [(64, 128, 2), (96, 160, 1)])
def test_validation_loss_matches_torch_cross_entropy(h, w, b):
    """BGModel.loss (bg_model.py:73-89, eval form) = fused upsample + CrossEntropyLoss(ignore_index=255) + accuracy,
    against torch on the full-resolution logits the same model returns."""
    import json
    import torch.nn.functional as F
    from panoptic_forecasting_amd import synth
    from panoptic_forecasting_amd.registry import build_model
    with open(os.path.join(G, 'calib_seed1234.json')) as f:
        sd = synth.make_state_dict(seed=1234, calib=json.load(f))
    params = {'task': 'bg', 'no_gpu': False, 'load_model': None, 'load_best_model': False,
              'data': {'num_classes': 11, 'depth_norm_params': [torch.tensor([20.]), torch.tensor([15.])]},
              'model': {'num_inputs': 3, 'use_depth_inps': True, 'convert2onehot': True, 'final_h': h, 'final_w': w,
                        'return_logits': True}}
    m = build_model(params)
    m.load_state_dict(sd)
    m.eval()
    inp = {k: v.cuda() for k, v in synth.make_bg_inputs(b=b, h=h, w=w, seed=3).items()}
    g = torch.Generator().manual_seed(9)
    lab = torch.randint(0, 12, (b, h, w), generator=g)
    lab[lab == 11] = 255                                   # ignored pixels
    out = m.predict(inp, None)
    logits = out['logits'].cpu()
    want_loss = F.cross_entropy(logits, lab, ignore_index=255)
    want_acc = (logits.argmax(1) == lab).sum().float() / (lab != 255).sum().float()
    got = m.loss(inp, {'seg': lab.cuda()})
    assert abs(got['loss'].item() - want_loss.item()) <= 1e-5 * max(1.0, abs(want_loss.item()))
    assert abs(got['accuracy'].item() - want_acc.item()) <= 1e-6
    got8 = m.loss(inp, {'seg': lab.to(torch.uint8).cuda()})    # u8 labels, same numbers, deterministic
    assert got8['loss'].item() == got['loss'].item() and got8['accuracy'].item() == got['accuracy'].item()


@pytest.mark.parametrize('u8', [False, True], ids=['i64_labels', 'u8_labels'])
def test_nan_depth_is_flagged_not_turned_into_zero(u8):
    """A NaN depth propagates through the reference's fp32 conv (hardnet.py:16-25) even under a zero mask (NaN * 0 = NaN); the
    stem's ReLU max would turn it into 0.  The stem raises PF_STATUS_RANGE instead, the forward is re-run on the fp32 path under
    the default policy, and 'ignore' leaves the flag readable."""
    from panoptic_forecasting_amd import synth
    h, w = 64, 128
    inp = synth.make_bg_inputs(b=1, h=h, w=w, seed=3)
    inp['depth'] = inp['depth'].clone()
    inp['depth'][0, 1, 20, 40] = float('nan')
    cu = {k: v.cuda() for k, v in inp.items()}
    if u8:
        cu['seg'] = cu['seg'].to(torch.uint8)        # selects the 2 x 2-outputs-per-lane stem
    m = _model(h, w, on_range_overflow='ignore')
    m.predict(cu, None)['seg']
    assert m.range_status() & 1
    m2 = _model(h, w)
    m2.predict(cu, None)['seg']
    assert m2.range_reruns == 1
