"""fg forecaster, host side (no GPU): parameters, checkpoints, registry, refused configurations, ABI argument errors, and the
float64 checker of tests/fg_ref64.py pinned to the reference's own float64 run (tests/golden/g8_fgnet.npz); its stage functions
pinned to forward64 itself, and every crafted weight set to the single operation tests/test_gpu_fg_stages.py claims it leaves."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fg_ref64 as R
from panoptic_forecasting_amd import lib as pflib
from panoptic_forecasting_amd.fg_model import FGModel
from panoptic_forecasting_amd.registry import build_model


@pytest.fixture(scope='module')
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, 'g8_fgnet.npz'))


def test_state_dict_keys_and_shapes_match_the_reference(fx):
    sd = FGModel(R.fg_params()).state_dict()
    assert list(sd.keys()) == list(fx['keys'])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(fx['shapes'])
    assert len(sd) == 52 and sum(v.numel() for v in sd.values()) > 22_000_000


def test_save_load_round_trip(tmp_path):
    a = FGModel(R.fg_params())
    a.load_state_dict(R.fill_weights(a.state_dict()))
    a.save(str(tmp_path / 'fg.pt'))
    b = FGModel(R.fg_params())
    b.load(str(tmp_path / 'fg.pt'))
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)


def test_registry_builds_fg_and_still_refuses_odom():
    m = build_model(R.fg_params())
    assert isinstance(m, FGModel) and not next(m.parameters()).is_cuda
    assert torch.equal(m.traj_std.detach(), torch.tensor([R.TRAJ_STD]))
    p = R.fg_params()
    p['task'] = 'odom'
    with pytest.raises(ValueError, match='outside'):
        build_model(p)


@pytest.mark.parametrize('key,value', [('rnn_type', 'lstm'), ('num_convlstm_layers', 1), ('num_traj_out_layers', 1),
                                       ('only_loc_feats', True), ('no_traj_inst_feats', True), ('no_mask_traj_feats', True),
                                       ('only_input_odometry', True), ('use_odometry', False), ('use_depth_inp', False),
                                       ('rnn_hidden', 64), ('traj_feat_channels', 8)])
def test_unsupported_configurations_are_refused(key, value):
    with pytest.raises(ValueError, match=key):
        FGModel(R.fg_params(**{key: value}))


def test_absent_switch_defaults_are_refused_too():
    p = R.fg_params()
    del p['model']['num_convlstm_layers']            # the reference's default is 1 layer
    with pytest.raises(ValueError, match='num_convlstm_layers'):
        FGModel(p)


def test_abi_argument_errors_without_a_gpu():
    L = pflib.load()
    need = ctypes.c_size_t()
    assert L.pf_fg_workspace(-1, 3, 3, 0, ctypes.byref(need)) == -1
    assert b'bad dims' in L.pf_last_error()
    assert L.pf_fg_workspace(4, 0, 3, 0, ctypes.byref(need)) == -1
    assert L.pf_fg_workspace(4, 3, 17, 0, ctypes.byref(need)) == -1
    assert L.pf_fg_workspace(4, 3, 3, 1, ctypes.byref(need)) == -5           # PF_EUNSUPPORTED
    assert L.pf_fg_workspace(0, 3, 3, 0, ctypes.byref(need)) == 0
    assert L.pf_fg_workspace(32, 3, 3, 0, ctypes.byref(need)) == 0
    assert need.value >= 32 * 9 * 256 * 196 * 4
    raw, packed = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.pf_fg_weights_size(0, ctypes.byref(raw), ctypes.byref(packed)) == 0
    assert raw.value == sum(v.numel() for v in FGModel(R.fg_params()).state_dict().values())
    assert packed.value > raw.value
    assert L.pf_fg_weights_size(2, ctypes.byref(raw), ctypes.byref(packed)) == -5
    # odometry shorter than T_in + T_out, refused before any device work (null buffers are never touched)
    assert L.pf_fg_forward(None, 0, 4, 3, 3, 5, *([None] * 14), None, 0, None) == -1
    assert b'odometry' in L.pf_last_error()
    assert L.pf_fg_forward(None, 0, 0, 3, 3, 6, *([None] * 14), None, 0, None) == 0      # N = 0: nothing enqueued


def test_float64_checker_reproduces_the_reference(fx):
    m = FGModel(R.fg_params())
    sd = R.fill_weights(m.state_dict())
    inputs, labels = R.make_inputs(0, list(fx['counts']))
    with torch.no_grad():
        out = R.forward64(sd, *R.forward_args(inputs, labels))
    for k in ('normalized_trajectory', 'unnormalized_trajectory', 'masks'):
        ref = fx[k + '64']
        assert out[k].shape == ref.shape
        assert np.abs(out[k].numpy() - ref).max() <= 1e-9 * (1 + np.abs(ref).max()), k
    for k in ('mask_feats', 'output_feats'):
        v = out[k].numpy().reshape(-1)[fx[k + '_idx']]
        assert np.abs(v - fx[k + '_val']).max() <= 1e-9, k


# ------------------------------------------------------------------------ the stage functions and the crafted weight sets
# (the references of tests/test_gpu_fg_stages.py; float64 on the CPU, at most 2 instances and 2 steps where a ConvLSTM runs)
@pytest.fixture(scope='module')
def base_sd():
    return R.fill_weights(FGModel(R.fg_params()).state_dict())


def _digest(inputs, labels):
    import hashlib
    h = hashlib.sha256()
    for d in (inputs, labels):
        for k in sorted(d):
            for t in d[k]:
                h.update(k.encode())
                h.update(str(t.dtype).encode())
                h.update(str(tuple(t.shape)).encode())
                h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize('case,counts,kw,want', [
    (0, [3, 2], {}, '222f372bf3fcb606beacd00b47c3fedc9a907577295b98e3e77f05d501f507db'),
    (7, [4], dict(t_out=1, odom_t=6, output_inds=0), 'f4fbdef318cb33aace816d4e8fd76a365f40662d9ce47c3f8803f50be4c9ca22'),
    (3, [1], dict(masked=False), '0764520247608bc61b42ec61a84207473e3f121db2df95a07b6bef4f6d94d4ae')])
def test_three_step_inputs_keep_their_bits(case, counts, kw, want):
    """sha256 over names, dtypes, shapes and bytes of every input, recorded before make_inputs learnt ``t_in`` / ``mask_mode``"""
    assert _digest(*R.make_inputs(case, counts, **kw)) == want
    assert _digest(*R.make_inputs(case, counts, t_in=3, mask_mode='fixture', **kw)) == want


def test_mask_modes():
    cat = lambda d, k: torch.cat(d[k]).float()
    inp, _ = R.make_inputs(1, [3], t_in=5, t_out=2, mask_mode='absent')
    assert cat(inp, 'bbox_masks')[2].sum() == 0 and cat(inp, 'bbox_vel_masks')[2].sum() == 0
    assert cat(inp, 'bbox_masks')[0].sum() == 5
    inp, _ = R.make_inputs(1, [3], t_in=6, t_out=2, mask_mode='alternate')
    dm = cat(inp, 'depth_masks')[:, :, 0]
    prod = dm[:, 1:] * dm[:, :-1]
    assert prod.sum() == 1 and prod[0, -1] == 1                  # 1 only where intended ...
    assert (dm[:, 1:] * (1 - dm[:, :-1])).sum() >= 6             # ... where dm alone is 1 at many steps: the two masks differ
    inp, lab = R.make_inputs(1, [3], t_in=4, t_out=2, mask_mode='wide')
    assert cat(inp, 'bbox_masks').shape == (3, 6) and cat(inp, 'bbox_vel_masks').shape == (3, 6)
    assert cat(inp, 'bbox_masks')[:, 4:].all() and cat(inp, 'bbox_vel_masks')[:, 4:].all()
    ref, _ = R.make_inputs(1, [3], t_in=4, t_out=2)
    for a, b in zip(R.forward_args(inp, lab), R.forward_args(ref, lab)):
        assert (torch.equal(a, b) if torch.is_tensor(a) else a == b)
    for t_in in (1, 2, 16):
        inp, lab = R.make_inputs(2, [4], t_in=t_in, t_out=1)
        assert R.forward_args(inp, lab)[3].shape == (4, t_in, 256, 14, 14) and R.forward_args(inp, lab)[5].shape == (4, t_in + 1, 5)


def test_stages_fed_with_forward64s_own_tensors_reproduce_it(base_sd):
    inputs, labels = R.make_inputs(20, [2], t_in=2, t_out=2, output_inds=[0, 1])
    args = R.forward_args(inputs, labels)
    trajs, m, vm, feats, inds, odom, depths, dmask, classes, t_out = args
    taps = {}
    with torch.no_grad():
        ref = R.forward64(base_sd, *args, taps=taps)
        tr = R.traj64(base_sd, trajs, m, vm, feats, odom, depths, dmask, t_out, ref['mask_feats'])
        assert torch.equal(tr['normalized_trajectory'], ref['normalized_trajectory'])
        assert torch.equal(tr['unnormalized_trajectory'], ref['unnormalized_trajectory'])
        assert torch.equal(tr['enc_tfeat'], taps['enc_tfeat'])
        assert torch.equal(R.gather64(ref['mask_feats'], inds), ref['output_feats'])
        assert torch.equal(ref['output_feats'][1], ref['mask_feats'][1, 2])
        assert torch.equal(R.head64(base_sd, ref['output_feats'], classes), ref['masks'])
        # the first cell: from the taps' own inputs, and its pre-activations
        x0 = torch.cat([taps['enc_tfeat'][:, 0, :, None, None].expand(-1, -1, 14, 14), feats[:, 0].double()], 1)
        z = torch.zeros(2, 256, 14, 14, dtype=torch.float64)
        h0, c0, pre = R.cell64(base_sd, 'mask_encoder.cell_list.0.conv', x0, z, z, gates=True)
        assert torch.equal(h0, taps['enc_l0'][0]) and all(torch.equal(a, b) for a, b in zip(pre, taps['cell0_pre'][0]))
        i, f, o, g = pre
        assert torch.equal(h0, torch.sigmoid(o) * torch.tanh(torch.sigmoid(i) * torch.tanh(g)))       # c_prev = 0: f does not enter
    # a different mask_feats moves the decoder slots and leaves slot 0 (the encoder's) alone
    with torch.no_grad():
        tr2 = R.traj64(base_sd, trajs, m, vm, feats, odom, depths, dmask, t_out, ref['mask_feats'] * 1.5)
    assert torch.equal(tr2['normalized_trajectory'][:, 0], ref['normalized_trajectory'][:, 0])
    assert not torch.equal(tr2['normalized_trajectory'][:, 1], ref['normalized_trajectory'][:, 1])


def _replicated(y):
    """[N, H, W] -> [N, 2H, 2W], every pixel four times"""
    return y.repeat_interleave(2, -2).repeat_interleave(2, -1)


@pytest.mark.parametrize('chans', [R.ONEHOT_A, R.ONEHOT_B], ids=['A', 'B'])
def test_crafted_head_sets_reduce_to_one_layer_exactly(base_sd, chans):
    """what tests/test_gpu_fg_stages.py claims of each crafted set, in float64, bit for bit"""
    n = 2
    of = R.sym(77, (n, 256, 14, 14), 1.0).double()              # both signs: the ReLU of an identity layer shows
    cls = torch.tensor([5, 2])
    ch = torch.tensor(chans)[cls]
    pick = lambda y: y[torch.arange(n), ch]
    ident = lambda ks: [('ident_fcn', k) for k in ks]
    F = torch.nn.functional
    w = lambda k: base_sd['mask_head.' + k].double()
    with torch.no_grad():
        # every fcn an identity, the deconv a replication, the predictor a selection: relu(output_feats)[ch], four times
        sd = R.crafted(base_sd, ident((1, 2, 3, 4)) + ['replicate_deconv', ('onehot_predictor', chans)])
        assert torch.equal(R.head64(sd, of, cls), _replicated(pick(F.relu(of))))
        # 2.1: mask_fcn1 alone / mask_fcn4 alone (its input is then relu(output_feats))
        sd = R.crafted(base_sd, ident((2, 3, 4)) + ['replicate_deconv', ('onehot_predictor', chans)])
        assert torch.equal(R.head64(sd, of, cls), _replicated(pick(F.relu(F.conv2d(of, w('mask_fcn1.weight'), w('mask_fcn1.bias'), padding=1)))))
        sd = R.crafted(base_sd, ident((1, 2, 3)) + ['replicate_deconv', ('onehot_predictor', chans)])
        assert torch.equal(R.head64(sd, of, cls),
                           _replicated(pick(F.relu(F.conv2d(F.relu(of), w('mask_fcn4.weight'), w('mask_fcn4.bias'), padding=1)))))
        # 2.2: the deconvolution alone
        sd = R.crafted(base_sd, ident((1, 2, 3, 4)) + [('onehot_predictor', chans)])
        assert torch.equal(R.head64(sd, of, cls), pick(F.relu(F.conv_transpose2d(F.relu(of), w('deconv.weight'), w('deconv.bias'), stride=2))))
        # 2.3: the predictor alone
        sd = R.crafted(base_sd, ident((1, 2, 3, 4)) + ['replicate_deconv'])
        y = _replicated(F.relu(of))
        want = torch.einsum('nchw,nc->nhw', y, w('predictor.weight')[cls, :, 0, 0]) + w('predictor.bias')[cls][:, None, None]
        assert torch.equal(R.head64(sd, of, cls), want)
    changed = sorted(k for k in sd if sd[k] is not base_sd[k])
    assert changed == sorted(['mask_head.mask_fcn%d.%s' % (k, p) for k in (1, 2, 3, 4) for p in ('weight', 'bias')] +
                             ['mask_head.deconv.weight', 'mask_head.deconv.bias'])


def test_crafted_cell_set_shows_cell_0_through_two_tanh(base_sd):
    """ident_out_conv + transparent_cell1 + const_traj_feat at one input step: mask_feats[:, 0] = s tanh(s tanh(h0)), s = sigmoid(20)
    (1 - 2.1e-9 in float64, exactly 1 in fp32), h0 = cell 0's output from c = 0 on [the bias planes, feats[:, 0]]"""
    sd = R.crafted(base_sd, ['ident_out_conv', 'transparent_cell1', ('const_traj_feat', 1.5)])
    inputs, labels = R.make_inputs(21, [1], t_in=1, t_out=1)
    args = R.forward_args(inputs, labels)
    taps = {}
    with torch.no_grad():
        out = R.forward64(sd, *args, taps=taps)
        assert torch.equal(taps['enc_tfeat'][:, 0], sd['traj_feat_out.bias'].double()[None])
        s = torch.sigmoid(torch.tensor(20.0, dtype=torch.float64))
        h0 = taps['enc_l0'][0]
        assert torch.equal(out['mask_feats'][:, 0], s * torch.tanh(s * torch.tanh(h0)))
        x0 = torch.cat([sd['traj_feat_out.bias'].double()[None, :, None, None].expand(1, -1, 14, 14), args[3][:, 0].double()], 1)
        z = torch.zeros(1, 256, 14, 14, dtype=torch.float64)
        assert torch.equal(R.cell64(sd, 'mask_encoder.cell_list.0.conv', x0, z, z)[0], h0)
    assert float(torch.sigmoid(torch.tensor(20.0))) == 1.0 and float(torch.exp(torch.tensor(-20.0, dtype=torch.float64))) < 2.0 ** -25
    assert 1 - float(s) < 2.1e-9


HOT_GAIN = 16.0


def test_hot_weights_saturate_the_first_cell(base_sd):
    """the condition of the saturated-regime test, on the float64 reference alone: >= 5 % of cell 0's pre-activations beyond +-10,
    the largest beyond +-20 (analytic standard deviation 0.40 * gain)"""
    inputs, labels = R.make_inputs(22, [1], t_in=1, t_out=1)
    taps, cold = {}, {}
    with torch.no_grad():
        R.forward64(R.crafted(base_sd, ('hot', HOT_GAIN)), *R.forward_args(inputs, labels), taps=taps)
        R.forward64(base_sd, *R.forward_args(inputs, labels), taps=cold)
    share, top = R.saturation(taps['cell0_pre'][0])
    print('gain %g: %.1f %% beyond +-10, max %.1f; std %.3f (base fill %.3f)' % (
        HOT_GAIN, 100 * share, top, float(torch.cat(taps['cell0_pre'][0]).std()), float(torch.cat(cold['cell0_pre'][0]).std())))
    assert share >= 0.05 and top > 20.0
    assert R.saturation(cold['cell0_pre'][0])[1] < 10.0          # the base fill never gets there


def test_stored_maps_rebuild_exactly():
    """The map overlays of the fixture round-trip through fg_ref64.seg_overlay / seg_from_overlay."""
    bg = R.background(1, 2).numpy()
    seg = bg.copy()
    seg[0, 100:140, 200:260] = 14001
    seg[1, 0:8, 0:8] = bg[1, 0:8, 0:8]          # an instance pixel that equals the background value
    for panoptic in (True, False):
        base = seg.copy()
        if panoptic:
            base[(base >= 11) & (base < 1000)] = 255
        assert np.array_equal(R.seg_from_overlay(R.seg_overlay(base, bg, panoptic), bg, panoptic), base)
