"""fg forecaster on the MI355X: pf_fg_forward against the reference's float64 run (g8_fgnet.npz), predict_panoptic /
predict_semantics against the reference's maps, and sizes the fixture lacks against the float64 checker (tests/fg_ref64.py)
evaluated on the GPU."""
import os

import numpy as np
import pytest
import torch

import fg_ref64 as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
OUTS = ('normalized_trajectory', 'unnormalized_trajectory', 'mask_feats', 'output_feats', 'masks')


@pytest.fixture(scope='module')
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, 'g8_fgnet.npz'))


@pytest.fixture(scope='module')
def model():
    from panoptic_forecasting_amd.registry import build_model
    p = R.fg_params()
    p['no_gpu'] = False
    m = build_model(p)
    m.load_state_dict(R.fill_weights(m.state_dict()))
    return m


@pytest.fixture(scope='module')
def sd64(model):
    return {k: v.detach().to(DEV, torch.float64) for k, v in model.state_dict().items()}


def _gpu_args(inputs, labels):
    return tuple(a.to(DEV) if torch.is_tensor(a) else a for a in R.forward_args(inputs, labels))


def _within(got, ref, tol, what):
    err = (got.double() - ref).abs().max().item() if got.numel() else 0.0
    assert err <= tol, '%s: max err %.3e > %.3e' % (what, err, tol)


def test_forward_matches_the_reference_float64(model, fx):
    inputs, labels = R.make_inputs(0, list(fx['counts']))
    out = model(*_gpu_args(inputs, labels))
    torch.cuda.synchronize()
    for k in ('normalized_trajectory', 'unnormalized_trajectory', 'masks'):
        ref = torch.from_numpy(fx[k + '64'].astype(np.float64))
        tol = 2 * float(fx[k + '_err32']) + 1e-6 * (1 + ref.abs().max().item())
        _within(out[k].cpu(), ref, tol, k)
    for k in ('mask_feats', 'output_feats'):            # seeded samples of the float64 tensors
        got = out[k].cpu().reshape(-1)[torch.from_numpy(fx[k + '_idx'])]
        tol = 2 * float(fx[k + '_err32']) + 1e-6 * (1 + float(fx[k + '_maxabs']))
        _within(got, torch.from_numpy(fx[k + '_val']), tol, k)


def _seg_agrees(got, ref):
    got = got.cpu().numpy().astype(np.int64)
    assert got.shape == ref.shape
    assert set(np.unique(got).tolist()) == set(np.unique(ref).tolist())
    assert (got != ref).mean() <= 1e-4


@pytest.mark.parametrize('method,key,sorting', [('predict_panoptic', 'seg_pan', False), ('predict_semantics', 'seg_sem', False),
                                                ('predict_panoptic', 'seg_pan_z', True)])
def test_predict_matches_the_reference_map(model, fx, method, key, sorting):
    inputs, labels = R.make_inputs(0, list(fx['counts']))
    inputs['background'] = list(R.background(1, len(fx['counts'])))
    model.merger.use_depth_sorting = sorting
    try:
        res = getattr(model, method)(inputs, labels)
    finally:
        model.merger.use_depth_sorting = False
    _seg_agrees(res['seg'], R.seg_from_overlay(fx[key + '_fg'], R.background(1, len(fx['counts'])).numpy(), key != 'seg_sem'))
    assert [b.shape for b in res['bbox']] == [(c, 3, 4) for c in fx['counts']]
    assert [d.shape for d in res['depths']] == [(c, 3) for c in fx['counts']]


@pytest.mark.parametrize('n,t_out,inds', [(1, 3, 0), (1, 3, 1), (1, 3, 2), (37, 1, None), (37, 3, None), (300, 3, None)])
def test_sizes_against_the_float64_checker(model, sd64, n, t_out, inds):
    inputs, labels = R.make_inputs(10 + n + t_out, [n], t_out=t_out, output_inds=inds)
    args = _gpu_args(inputs, labels)
    out = model(*args)
    with torch.no_grad():
        ref = R.forward64(sd64, *args)
    assert out['mask_feats'].shape == (n, 1 + t_out, 256, 14, 14) and out['masks'].shape == (n, 28, 28)
    for k in OUTS:
        _within(out[k], ref[k], 1e-5 * (1 + ref[k].abs().max().item()), '%s (N=%d, T_out=%d)' % (k, n, t_out))


def test_no_instances(model):
    inputs, labels = R.make_inputs(3, [0, 0])
    out = model(*_gpu_args(inputs, labels))
    assert out['masks'].shape == (0, 28, 28) and out['mask_feats'].shape == (0, 4, 256, 14, 14)
    bg = R.background(2, 2)
    inputs['background'] = list(bg)
    seg = model.predict_panoptic(inputs, labels)['seg'].cpu()
    want = bg.clone()
    want[want >= 11] = 255
    assert torch.equal(seg.long(), want)


def test_two_runs_are_bit_identical(model):
    args = _gpu_args(*R.make_inputs(4, [5, 4]))
    a = model(*args)
    b = model(*args)
    for k in OUTS:
        assert torch.equal(a[k], b[k]), k


def test_inputs_are_not_modified(model):
    args = _gpu_args(*R.make_inputs(5, [6]))
    before = [a.clone() if torch.is_tensor(a) else a for a in args]
    model(*args)
    torch.cuda.synchronize()
    for x, y in zip(args, before):
        assert (torch.equal(x, y) if torch.is_tensor(x) else x == y)


def test_captured_forward_replays_bit_identical(model):
    args = _gpu_args(*R.make_inputs(6, [7, 5]))
    eager = model(*args)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model(*args)                                       # warm-up on the capture stream (workspace, packed weights)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = model(*args)
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    for k in OUTS:
        assert torch.equal(cap[k], eager[k]), k


def test_weights_are_repacked_after_load(model, tmp_path):
    args = _gpu_args(*R.make_inputs(7, [3]))
    a = model(*args)['masks'].clone()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    changed = {k: (v * 0.5 if k == 'mask_head.predictor.weight' else v) for k, v in sd.items()}
    model.load_state_dict(changed)
    try:
        b = model(*args)['masks'].clone()
    finally:
        model.load_state_dict(sd)
    c = model(*args)['masks']
    assert not torch.equal(a, b) and torch.equal(a, c)
