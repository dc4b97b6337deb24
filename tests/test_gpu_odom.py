"""odometry forecaster on the MI355X: pf_odom_forward against the reference's float64 run (g9_odomnet.npz), sizes the
fixture lacks against the float64 checker (tests/odom_ref64.py) evaluated on the GPU, batch independence, graph replay,
re-packing and the export driver against the reference's own export."""
import os

import numpy as np
import pytest
import torch

import odom_ref64 as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, 'g9_odomnet.npz'))


def _model(mode):
    from panoptic_forecasting_amd.registry import build_model
    p = R.odom_params(predict_type=mode)
    p['no_gpu'] = False
    m = build_model(p)
    m.load_state_dict(R.fill_weights(m.state_dict()))
    return m


@pytest.fixture(scope='module')
def models():
    return {mode: _model(mode) for mode in ('direct', 'offset')}


def _within(got, ref, tol, what):
    err = (got.double() - ref).abs().max().item() if got.numel() else 0.0
    assert err <= tol, '%s: max err %.3e > %.3e' % (what, err, tol)


@pytest.mark.parametrize('mode', ['direct', 'offset'])
def test_forward_matches_the_reference_float64(models, fx, mode):
    out, norm = models[mode](R.make_inputs(0, 32).to(DEV), 9)
    torch.cuda.synchronize()
    for got, key in ((out, '_out'), (norm, '_norm')):
        ref = torch.from_numpy(fx[mode + key + '64'])
        tol = 2 * float(fx[mode + key + '_err32']) + 1e-6 * (1 + ref.abs().max().item())
        _within(got.cpu(), ref, tol, mode + key)


@pytest.mark.parametrize('b,t_in,t_out,mode', [(1, 9, 9, 'direct'), (15, 2, 1, 'offset'), (16, 64, 9, 'direct'),
                                               (17, 9, 64, 'offset'), (33, 2, 64, 'direct'), (4097, 9, 1, 'offset'),
                                               (12000, 9, 9, 'direct'), (12000, 64, 64, 'offset')])
def test_sizes_against_the_float64_checker(models, b, t_in, t_out, mode):
    m = models[mode]
    x = R.make_inputs(10 + t_in + t_out, b, t_in).to(DEV)
    out, norm = m(x, t_out)
    sd64 = {k: v.detach().double() for k, v in m.state_dict().items()}
    ref, ref_n = R.forward64(sd64, x, t_out, mode)
    assert out.shape == norm.shape == (b, t_out, 2)
    _within(out, ref, 1e-5 * (1 + ref.abs().max().item()), 'out (B=%d, T_in=%d, T_out=%d, %s)' % (b, t_in, t_out, mode))
    _within(norm, ref_n, 1e-5 * (1 + ref_n.abs().max().item()), 'norm (B=%d, T_in=%d, T_out=%d, %s)' % (b, t_in, t_out, mode))


def test_empty_batch_launches_nothing(models):
    from panoptic_forecasting_amd import lib as pflib
    m = models['direct']
    out, norm = m(torch.zeros(0, 9, 2, device=DEV), 9)
    assert out.shape == norm.shape == (0, 9, 2)
    pflib.profile(True)
    try:
        m(torch.zeros(0, 9, 2, device=DEV), 9)
        recs = pflib.profile_results()
        m(R.make_inputs(3, 3).to(DEV), 9)                # a forecast is one launch
        one = pflib.profile_results()
    finally:
        pflib.profile(False)
    assert not [r for r in recs if r['launches']], recs
    assert [(r['label'], r['launches']) for r in one if r['launches']] == [('pf::odom::odom_forward_kernel', 1)], one


def test_two_runs_are_bit_identical(models):
    x = R.make_inputs(4, 70).to(DEV)
    for m in models.values():
        a, an = m(x, 9)
        b, bn = m(x, 9)
        assert torch.equal(a, b) and torch.equal(an, bn)


def test_rows_do_not_depend_on_the_batch(models):
    big = R.make_inputs(5, 12000).to(DEV)
    for m in models.values():
        out, norm = m(big, 9)
        for i in (0, 47, 48, 4096, 11999):
            alone, alone_n = m(big[i:i + 1].clone(), 9)
            assert torch.equal(alone[0], out[i]) and torch.equal(alone_n[0], norm[i]), i
        part, _ = m(big[17:50].clone(), 9)
        assert torch.equal(part, out[17:50])


def test_inputs_are_not_modified(models):
    x = R.make_inputs(6, 40).to(DEV)
    before = x.clone()
    models['offset'](x, 9)
    torch.cuda.synchronize()
    assert torch.equal(x, before)


def test_captured_predict_replays_bit_identical(models):
    m = models['direct']
    inputs = {'odometry': R.make_inputs(7, 45).to(DEV)}
    labels = {'odometry': torch.zeros(45, 9, 2, device=DEV)}
    eager = m.predict(inputs, labels)['odometry'].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.predict(inputs, labels)                       # warm-up on the capture stream (packed weights)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = m.predict(inputs, labels)['odometry']
    for _ in range(5):
        cap.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap, eager)


def test_weights_are_repacked_after_load(models):
    m = models['direct']
    x = R.make_inputs(8, 20).to(DEV)
    a = m(x, 9)[0].clone()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    changed = {k: (v * 0.5 if k == 'rnn.weight_hh_l0' else v) for k, v in sd.items()}
    m.load_state_dict(changed)
    try:
        b = m(x, 9)[0].clone()
    finally:
        m.load_state_dict(sd)
    c = m(x, 9)[0]
    assert not torch.equal(a, b) and torch.equal(a, c)


def test_export_matches_the_reference_export(fx, models, tmp_path):
    pd = pytest.importorskip('pandas')
    import yaml
    from panoptic_forecasting_amd import export_odom, odom_io
    data_dir = tmp_path / 'meta'
    data_dir.mkdir()
    pd.DataFrame({'city': list(fx['snip_city']), 'seq': list(fx['snip_seq']), 'frame': list(fx['snip_frame']),
                  'odometry': list(fx['snip_odometry'])}).to_pickle(str(data_dir / 'val_3d_info.pkl'))
    work = tmp_path / 'work'
    work.mkdir()
    models['direct'].save(str(work / 'odom_model.pt'))
    cfg = {'task': 'odom', 'model': dict(R.ODOM_CONFIG),
           'data': {'dataset_type': 'odom', 'data_splits': ['val'], 'data_dir': str(data_dir)},
           'training': {'batch_size': 32}}
    with open(str(work / 'config.yaml'), 'w') as f:
        yaml.safe_dump(cfg, f)
    export_odom.main(['--load_model', str(work / 'odom_model.pt'), '--working_dir', str(work)])
    path = work / 'odometry_val.npz'
    with np.load(str(path)) as z:
        names = sorted(z.files)
        got = np.stack([z[n] for n in fx['export_names']])
    assert names == sorted(fx['export_names'])
    ref = fx['export_data']
    tol = 3 * float(fx['export_err32']) + 1e-6 * (1 + np.abs(ref).max())
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.abs(got.astype(np.float64) - ref).max() <= tol
    # the consumers: OdometryFile opens the .npz twin of the reference's .h5 name, the ego chain takes a snippet's rows
    with odom_io.OdometryFile(str(work / 'odometry_val.h5')) as f:
        rows = f.rows('bonn', '000041', 33, 16)
    assert np.array_equal(rows, got[list(fx['export_names']).index('bonn/000041/33/16')])
    cs = tmp_path / 'cityscapes'
    rng = np.random.Generator(np.random.PCG64(5))
    for fr in range(33 - 19, 33 + 11):
        for sub, name, text in (('timestamp_sequence', '_timestamp.txt', '%d' % int(1.5e18 + fr * 5.8e7)),
                                ('vehicle_sequence', '_vehicle.json',
                                 '{"speed": %.4f, "yawRate": %.5f}' % (rng.uniform(2, 12), rng.normal(0, 0.05)))):
            d = cs / sub / 'val' / 'bonn'
            d.mkdir(parents=True, exist_ok=True)
            (d / ('bonn_000041_%06d%s' % (fr, name))).write_text(text)
    with odom_io.OdometryFile(str(path)) as f:
        T = odom_io.snippet_target_T(str(cs), 'val', 'bonn', '000041', 33, 3, odom=f)
    assert T.shape == (3, 4, 4) and np.isfinite(T).all()
