"""odom training on the MI355X: ``forward_train`` against ``forward`` bit for bit, ``OdomModel.loss`` and its gradients
(pf_odom_backward) against float64 autograd of the checker (tests/odom_train_ref.py) and against the reference's own
gradients (g10_odomtrain.npz), row independence, determinism, accumulation, graph replay, an SGD trajectory and the
training driver.

The gradient bar: per tensor max|g - g64| <= 2 * max|g32 - g64| + 1e-6 * max|g64|, per-sequence losses
2 * err32 + 1e-6 * (1 + |loss64|), where g32 / err32 come from the same checker run in torch fp32 on the same device
inside the test.  The factor 2 is the project's criterion for training kernels; the floor is 16 fp32 ulps of the largest
element (torch's own error is sometimes luckily tiny).  Every figure is printed before it is asserted (pytest -s).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import odom_ref64 as R
import odom_train_ref as T

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
_MODELS = {}


@pytest.fixture(scope='module')
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, 'g10_odomtrain.npz'))


def model_for(mode, loss_fn='mse', normalised=True):
    key = (mode, loss_fn, normalised)
    if key not in _MODELS:
        from panoptic_forecasting_amd.registry import build_model
        p = R.odom_params(predict_type=mode, loss_fn=loss_fn, use_normalized_loss=normalised)
        p['no_gpu'] = False
        _MODELS[key] = build_model(p)
    m = _MODELS[key]
    m.load_state_dict(R.fill_weights(m.state_dict()))
    for k, p in m.named_parameters():
        p.requires_grad_(k in T.TRAINABLE)
        p.grad = None
    return m


def native(m, x, y, weights=None):
    """(losses [B], {key: grad}) of sum_b weights_b * loss_b (default: the mean) through OdomModel.loss."""
    for p in m.parameters():
        p.grad = None
    loss = m.loss({'odometry': x}, {'odometry': y})['loss']
    assert loss.grad_fn is not None and loss.shape == (x.shape[0],)
    (loss.mean() if weights is None else (loss * weights).sum()).backward()
    return loss.detach(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def checkers(m, x, y, mode, loss_fn, normalised, weights=None):
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    return (T.loss_and_grads(sd, x, y, mode, loss_fn, normalised, torch.float64, weights),
            T.loss_and_grads(sd, x, y, mode, loss_fn, normalised, torch.float32, weights))


def within_bar(what, loss, grads, ref64, ref32):
    (l64, g64), (l32, g32) = ref64, ref32
    misses = []
    if loss is not None:
        err, err32 = (loss.double() - l64).abs().max().item(), (l32.double() - l64).abs().max().item()
        tol = 2 * err32 + 1e-6 * (1 + l64.abs().max().item())
        print('%s loss: err %.3e  torch fp32 %.3e  bar %.3e' % (what, err, err32, tol))
        if not err <= tol:
            misses.append('loss %.3e > %.3e' % (err, tol))
    assert sorted(grads) == sorted(T.TRAINABLE)
    for k in T.TRAINABLE:
        big = g64[k].abs().max().item()
        err, err32 = (grads[k].double() - g64[k]).abs().max().item(), (g32[k].double() - g64[k]).abs().max().item()
        tol = 2 * err32 + 1e-6 * big
        print('%s %-18s err/max %.3e  torch fp32 %.3e  bar %.3e' % (what, k, err / big, err32 / big, tol / big))
        if not err <= tol:
            misses.append('%s %.3e > %.3e' % (k, err, tol))
    assert not misses, '%s: %s' % (what, '; '.join(misses))


# ------------------------------------------------------------------------------------------------ forward_train = forward
@pytest.mark.parametrize('mode', ['direct', 'offset'])
@pytest.mark.parametrize('t_in,t_out', [(9, 9), (2, 1), (64, 64)])
@pytest.mark.parametrize('b', [1, 17, 97, 4097])
def test_forward_train_is_forward_bit_for_bit(b, t_in, t_out, mode):
    m = model_for(mode)
    x = R.make_inputs(20 + t_in + t_out, b, t_in).to(DEV)
    out, norm = m(x, t_out)
    out_t, norm_t = m.forward_train(x, t_out)
    assert out_t.grad_fn is not None and norm_t.grad_fn is not None
    assert torch.equal(out_t, out) and torch.equal(norm_t, norm)


def test_training_launch_has_its_own_label_and_inference_keeps_its_own():
    from panoptic_forecasting_amd import lib as pflib
    m = model_for('direct')
    x, y = R.make_inputs(3, 5).to(DEV), T.make_labels(3, 5).to(DEV)
    m(x, 9)                                              # packs the weights outside the profile
    pflib.profile(True)
    try:
        m(x, 9)
        inference = pflib.profile_results()
        native(m, x, y)
        training = pflib.profile_results()
    finally:
        pflib.profile(False)
    assert [(r['label'], r['launches']) for r in inference if r['launches']] == [('pf::odom::odom_forward_kernel', 1)]
    labels = {r['label']: r['launches'] for r in training if r['launches']}
    # the records run on from profile(True): the inference launch is still there, once
    assert labels == {'pf::odom::odom_forward_kernel': 1, 'pf::odom::odom_train_forward_kernel': 1,
                      'pf::odom::odom_bptt_kernel': 1, 'pf::odom::odom_wgrad_kernel': 1,
                      'pf::odom::odom_wgrad_reduce_kernel': 1}, training


def test_inps_requiring_grad_are_refused():
    m = model_for('direct')
    with pytest.raises(ValueError, match='requires_grad'):
        m.forward_train(R.make_inputs(3, 5).to(DEV).requires_grad_(), 9)


# ------------------------------------------------------------------------------------------------ gradients
GRAD_CASES = [(1, 9, 9, 'direct', 'mse', True), (15, 2, 1, 'offset', 'smooth_l1', False), (16, 64, 9, 'direct', 'mse', True),
              (17, 9, 64, 'offset', 'mse', True), (33, 2, 64, 'direct', 'smooth_l1', True),
              (97, 9, 9, 'direct', 'smooth_l1', True), (4097, 9, 9, 'offset', 'mse', False)]


@pytest.mark.parametrize('b,t_in,t_out,mode,loss_fn,normalised', GRAD_CASES)
def test_loss_and_gradients_against_float64_autograd(b, t_in, t_out, mode, loss_fn, normalised):
    m = model_for(mode, loss_fn, normalised)
    case = 30 + t_in + t_out
    x, y = R.make_inputs(case, b, t_in).to(DEV), T.make_labels(case, b, t_out).to(DEV)
    loss, grads = native(m, x, y)
    ref64, ref32 = checkers(m, x, y, mode, loss_fn, normalised)
    within_bar('B=%d %d/%d %s %s %s' % (b, t_in, t_out, mode, loss_fn, normalised), loss, grads, ref64, ref32)


@pytest.mark.parametrize('cfg,mode,loss_fn,normalised', T.CONFIGS)
def test_gradients_against_the_reference(fx, cfg, mode, loss_fn, normalised):
    m = model_for(mode, loss_fn, normalised)
    x, y = R.make_inputs(0, 32).to(DEV), T.make_labels(0, 32).to(DEV)
    loss, grads = native(m, x, y)
    _, ref32 = checkers(m, x, y, mode, loss_fn, normalised)
    ref64 = (torch.from_numpy(fx[cfg + '_loss64']).to(DEV),
             {k: torch.from_numpy(fx[cfg + '_grad_' + k]).to(DEV) for k in T.TRAINABLE})
    within_bar('reference ' + cfg, loss, grads, ref64, ref32)


@pytest.mark.parametrize('i', [0, 16, 96])
def test_one_hot_grad_gives_that_sequences_gradients(i):
    mode, loss_fn, normalised = 'offset', 'mse', True
    m = model_for(mode, loss_fn, normalised)
    x, y = R.make_inputs(40, 97).to(DEV), T.make_labels(40, 97).to(DEV)
    hot = torch.zeros(97, device=DEV)
    hot[i] = 1.0
    _, grads = native(m, x, y, hot)
    one = torch.ones(1, device=DEV)
    ref64, ref32 = checkers(m, x[i:i + 1], y[i:i + 1], mode, loss_fn, normalised, one)
    within_bar('one-hot %d of 97' % i, None, grads, ref64, ref32)
    _, alone = native(m, x[i:i + 1].clone(), y[i:i + 1].clone(), one)
    within_bar('B=1 of row %d' % i, None, alone, ref64, ref32)


def test_two_backward_runs_are_bit_identical():
    for mode, b in (('direct', 97), ('offset', 4097)):
        m = model_for(mode)
        x, y = R.make_inputs(41, b).to(DEV), T.make_labels(41, b).to(DEV)
        la, ga = native(m, x, y)
        lb, gb = native(m, x, y)
        assert torch.equal(la, lb)
        for k in T.TRAINABLE:
            assert torch.equal(ga[k], gb[k]), k


def test_two_backwards_without_zero_grad_accumulate_exactly():
    m = model_for('direct')
    x, y = R.make_inputs(42, 33).to(DEV), T.make_labels(42, 33).to(DEV)
    _, g = native(m, x, y)
    for p in m.parameters():
        p.grad = None
    for _ in range(2):
        m.loss({'odometry': x}, {'odometry': y})['loss'].mean().backward()
    for k, p in m.named_parameters():
        if k in T.TRAINABLE:
            assert torch.equal(p.grad, 2 * g[k]), k
        else:
            assert p.grad is None, k


def test_a_second_backward_of_one_forward_is_refused():
    m = model_for('direct')
    x, y = R.make_inputs(42, 8).to(DEV), T.make_labels(42, 8).to(DEV)
    loss = m.loss({'odometry': x}, {'odometry': y})['loss'].mean()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='one backward per'):
        loss.backward()
    first = m.loss({'odometry': x}, {'odometry': y})['loss'].mean()
    m.loss({'odometry': x}, {'odometry': y})                     # the same shape: reuses the workspace
    with pytest.raises(RuntimeError, match='one backward per'):
        first.backward()


def test_frozen_parameters_get_no_grad():
    m = model_for('offset')
    m.rnn.bias_hh_l0.requires_grad_(False)
    m.out[0].weight.requires_grad_(False)
    x, y = R.make_inputs(43, 20).to(DEV), T.make_labels(43, 20).to(DEV)
    _, grads = native(m, x, y)
    assert sorted(grads) == sorted(k for k in T.TRAINABLE if k not in ('rnn.bias_hh_l0', 'out.0.weight'))
    assert m.odom_mean.grad is None and m.odom_std.grad is None
    ref64, ref32 = checkers(m, x, y, 'offset', 'mse', True)
    for k in grads:                                              # the others are what they are with everything trainable
        tol = 2 * (ref32[1][k].double() - ref64[1][k]).abs().max().item() + 1e-6 * ref64[1][k].abs().max().item()
        assert (grads[k].double() - ref64[1][k]).abs().max().item() <= tol, k


def test_inputs_and_labels_are_not_modified():
    m = model_for('offset', 'smooth_l1', False)
    x, y = R.make_inputs(44, 40).to(DEV), T.make_labels(44, 40).to(DEV)
    x0, y0 = x.clone(), y.clone()
    native(m, x, y)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and torch.equal(y, y0)


def test_empty_batch_gives_an_empty_loss_without_a_launch():
    from panoptic_forecasting_amd import lib as pflib
    m = model_for('direct')
    m(R.make_inputs(3, 3).to(DEV), 9)                            # packs the weights outside the profile
    x, y = torch.zeros(0, 9, 2, device=DEV), torch.zeros(0, 9, 2, device=DEV)
    pflib.profile(True)
    try:
        loss = m.loss({'odometry': x}, {'odometry': y})['loss']
        recs = pflib.profile_results()
    finally:
        pflib.profile(False)
    assert loss.shape == (0,) and loss.grad_fn is not None
    assert not [r for r in recs if r['launches']], recs
    loss.sum().backward()                                        # only the zero fill of grad_raw
    for k, p in m.named_parameters():
        if k in T.TRAINABLE:
            assert p.grad is not None and not p.grad.any(), k


# ------------------------------------------------------------------------------------------------ the ABI under capture
def test_captured_forward_and_backward_replay_bit_identical():
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    m = model_for('offset')
    b, t_in, t_out, flags = 45, 9, 9, 1
    packed = m.packed_weights()
    x = R.make_inputs(45, b).to(DEV)
    go, gon = T.make_labels(45, b).to(DEV) * 0.01, T.make_labels(46, b).to(DEV) * 0.01
    n = ctypes.c_size_t()
    pflib.check(L.pf_odom_train_workspace(b, t_in, t_out, flags, ctypes.byref(n)), 'pf_odom_train_workspace')
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    out, norm = torch.empty(b, t_out, 2, device=DEV), torch.empty(b, t_out, 2, device=DEV)
    grad = torch.empty(50950, device=DEV)

    def run():
        s = pflib.stream_ptr()
        pflib.check(L.pf_odom_train_forward(packed.data_ptr(), flags, b, t_in, t_out, x.data_ptr(), out.data_ptr(),
                                            norm.data_ptr(), ws.data_ptr(), n.value, s), 'pf_odom_train_forward')
        pflib.check(L.pf_odom_backward(packed.data_ptr(), flags, b, t_in, t_out, x.data_ptr(), norm.data_ptr(), go.data_ptr(),
                                       gon.data_ptr(), ws.data_ptr(), n.value, grad.data_ptr(), s), 'pf_odom_backward')
    run()
    torch.cuda.synchronize()
    eager = [t.clone() for t in (out, norm, grad)]
    assert eager[2][4:].abs().max() > 0 and not eager[2][:4].any()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                    # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        run()
    for _ in range(5):
        for t in (out, norm, grad):
            t.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        for got, ref in zip((out, norm, grad), eager):
            assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------ a trajectory
@pytest.mark.parametrize('mode', ['direct', 'offset'])
def test_ten_sgd_steps_follow_the_float64_checker(mode):
    m = model_for(mode)
    x, y = R.make_inputs(50, 64).to(DEV), T.make_labels(50, 64).to(DEV)

    def checker_run(dtype):
        leaves = {k: v.detach().to(dtype).clone().requires_grad_(k in T.TRAINABLE) for k, v in m.state_dict().items()}
        opt = torch.optim.SGD([leaves[k] for k in T.TRAINABLE], lr=0.01, momentum=0.9)
        losses = []
        for _ in range(10):
            opt.zero_grad()
            loss = T.loss_ref(leaves, x, y, mode, 'mse', True, dtype).mean()
            loss.backward()
            opt.step()
            losses.append(loss.item())
        return losses, {k: leaves[k].detach() for k in T.TRAINABLE}
    l64, p64 = checker_run(torch.float64)
    l32, p32 = checker_run(torch.float32)
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=0.01, momentum=0.9)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = m.loss({'odometry': x}, {'odometry': y})['loss'].mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print('%s losses %.6f -> %.6f (float64 %.6f -> %.6f)' % (mode, losses[0], losses[-1], l64[0], l64[-1]))
    assert l64[-1] < l64[0]
    misses = []
    for i, (a, b32, b64) in enumerate(zip(losses, l32, l64)):
        tol = 2 * abs(b32 - b64) + 1e-6 * abs(b64)
        print('step %d loss err %.3e  torch fp32 %.3e  bar %.3e' % (i, abs(a - b64), abs(b32 - b64), tol))
        if not abs(a - b64) <= tol:
            misses.append('loss %d: %.3e > %.3e' % (i, abs(a - b64), tol))
    got = dict(m.named_parameters())
    for k in T.TRAINABLE:
        big = p64[k].abs().max().item()
        err, err32 = (got[k].detach().double() - p64[k]).abs().max().item(), (p32[k].double() - p64[k]).abs().max().item()
        tol = 2 * err32 + 1e-6 * big
        print('%-18s err/max %.3e  torch fp32 %.3e  bar %.3e' % (k, err / big, err32 / big, tol / big))
        if not err <= tol:
            misses.append('%s %.3e > %.3e' % (k, err, tol))
    assert not misses, '; '.join(misses)


# ------------------------------------------------------------------------------------------------ the driver
def test_train_odom_synthetic_writes_resumes_and_exports(tmp_path, capsys):
    pd = pytest.importorskip('pandas')
    import yaml
    from panoptic_forecasting_amd import export_odom, train_odom
    meta = tmp_path / 'meta'
    meta.mkdir()
    snips = train_odom.synthetic_snippets(2, seed=5)
    pd.DataFrame({'city': ['bonn', 'ulm'], 'seq': ['000041', '000007'], 'frame': [33, 25],
                  'odometry': list(snips)}).to_pickle(str(meta / 'val_3d_info.pkl'))
    cfg = {'task': 'odom', 'model': dict(R.ODOM_CONFIG),
           'data': {'dataset_type': 'odom', 'data_splits': ['val'], 'data_dir': str(meta)},
           'training': {'batch_size': 32, 'num_epochs': 2, 'lr': 5.0e-4, 'clip_grad_norm': 5.0, 'use_adam': True}}
    with open(str(tmp_path / 'odom_train.yaml'), 'w') as f:
        yaml.safe_dump(cfg, f)
    work = tmp_path / 'work'
    train_odom.main(['--config_file', str(tmp_path / 'odom_train.yaml'), '--working_dir', str(work), '--synthetic', '8'])
    for name in ('config.yaml', 'model_checkpoint', 'best_model', 'training_checkpoint'):
        assert (work / name).exists(), name
    st = torch.load(str(work / 'training_checkpoint'), map_location='cpu')
    assert st['epoch'] == 3 and st['step'] == 2 * (8 * 15 // 32) and st['best_val_epoch'] in (1, 2)
    assert sorted(st) == ['best_val_epoch', 'best_val_result', 'epoch', 'optimizer', 'step']
    best = torch.load(str(work / 'best_model'), map_location='cpu')
    fresh = R.fill_weights({k: v for k, v in model_for('direct').state_dict().items()})
    assert list(best.keys()) == list(fresh.keys()) and all(best[k].shape == fresh[k].shape for k in best)
    mean, std = train_odom.norm_params(train_odom.synthetic_snippets(8))
    assert torch.equal(best['odom_mean'], mean[None]) and torch.equal(best['odom_std'], std[None])
    capsys.readouterr()
    train_odom.main(['--continue_training', '--working_dir', str(work), '--synthetic', '8',
                     '--extra_args', 'training.num_epochs', '3'])
    assert 'STARTING EPOCH:  3' in capsys.readouterr().out
    st = torch.load(str(work / 'training_checkpoint'), map_location='cpu')
    assert st['epoch'] == 4 and st['step'] == 3 * (8 * 15 // 32)
    export_odom.main(['--load_best_model', '--working_dir', str(work)])
    with np.load(str(work / 'odometry_val.npz')) as z:
        assert len(z.files) == 2 * 24 and z['bonn/000041/33/8'].shape == (9, 2) and np.isfinite(z['bonn/000041/33/8']).all()
