"""fg forecaster, host side (no GPU): parameters, checkpoints, registry, refused configurations, ABI argument errors, and the
float64 checker of tests/fg_ref64.py pinned to the reference's own float64 run (tests/golden/g8_fgnet.npz)."""
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
