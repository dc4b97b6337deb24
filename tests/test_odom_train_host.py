"""odom training, host side (no GPU): the training windows and normalisation parameters, the float64 loss checker of
tests/odom_train_ref.py pinned to the reference's own ``loss()`` and gradients in tests/golden/g10_odomtrain.npz, the
argument checks of the training entry points, and ``loss`` on a host model."""
import ctypes
import os

import numpy as np
import pytest
import torch

import odom_ref64 as R
import odom_train_ref as T
from panoptic_forecasting_amd import lib as pflib
from panoptic_forecasting_amd import odom_io, train_odom
from panoptic_forecasting_amd.odom_model import OdomModel


@pytest.fixture(scope='module')
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, 'g10_odomtrain.npz'))


def test_training_windows_reproduce_the_reference_dataset(fx):
    wins = [odom_io.odom_windows(odo, test=False) for odo in fx['snip_odometry']]
    inputs, labels, starts = (np.concatenate([w[j] for w in wins]) for j in range(3))
    assert inputs.dtype == labels.dtype == np.float32 and len(starts) == 3 * 15
    assert np.array_equal(inputs, fx['win_inputs']) and np.array_equal(labels, fx['win_labels'])
    assert np.array_equal(starts, fx['win_start'])
    assert list(starts[:15]) == list(range(8, 21)) + [7, 6]


def test_default_windows_are_the_export_windows(fx):
    odo = fx['snip_odometry'][0]
    for a, b in zip(odom_io.odom_windows(odo), odom_io.odom_windows(odo, test=True)):
        assert np.array_equal(a, b)
    assert len(odom_io.odom_windows(odo)[2]) == 24
    assert len(odom_io.odom_windows(odo, test=False)[2]) == 30 - 18 + 1 + 2


def test_norm_params_reproduce_the_reference_dataset(fx):
    mean, std = train_odom.norm_params(fx['snip_odometry'])
    assert mean.dtype == std.dtype == torch.float32
    assert np.array_equal(mean.numpy(), fx['norm_mean']) and np.array_equal(std.numpy(), fx['norm_std'])


@pytest.mark.parametrize('cfg,mode,loss_fn,normalised', T.CONFIGS)
def test_loss_checker_reproduces_the_reference(fx, cfg, mode, loss_fn, normalised):
    sd = R.fill_weights(OdomModel(R.odom_params()).state_dict())
    loss, grads = T.loss_and_grads(sd, R.make_inputs(0, 32), T.make_labels(0, 32), mode, loss_fn, normalised)
    ref = fx[cfg + '_loss64']
    assert loss.shape == ref.shape == (32,)
    assert np.abs(loss.numpy() - ref).max() <= 1e-12 * np.abs(ref).max()
    for k in T.TRAINABLE:
        g = fx[cfg + '_grad_' + k]
        assert grads[k].shape == g.shape and np.abs(g).max() > 0
        assert np.abs(grads[k].numpy() - g).max() <= 1e-12 * np.abs(g).max(), k


def test_train_abi_argument_errors_without_a_gpu():
    L = pflib.load()
    n = ctypes.c_size_t()
    junk = ctypes.create_string_buffer(64)
    assert L.pf_odom_train_workspace(4, 9, 9, 0, None) == -1
    assert L.pf_odom_train_workspace(4, 9, 9, 2, ctypes.byref(n)) == -5                       # PF_EUNSUPPORTED
    # dimensions and buffers are checked before any device work: the junk buffers below are never touched
    for b, t_in, t_out in ((4, 1, 9), (4, 9, 0), (-1, 9, 9), (4, 65, 9), (4, 9, 65)):
        assert L.pf_odom_train_workspace(b, t_in, t_out, 0, ctypes.byref(n)) == -1
        assert L.pf_odom_train_forward(None, 0, b, t_in, t_out, None, None, None, None, 0, None) == -1
        assert b'bad dims' in L.pf_last_error()
        assert L.pf_odom_backward(None, 0, b, t_in, t_out, None, None, None, None, None, 0, junk, None) == -1
        assert b'bad dims' in L.pf_last_error()
    assert L.pf_odom_train_workspace(4, 9, 9, 0, ctypes.byref(n)) == 0
    big = n.value
    for miss in range(5):                                   # packed, inps, out, out_norm, ws
        args = [junk] * 5
        args[miss] = None
        assert L.pf_odom_train_forward(args[0], 0, 4, 9, 9, args[1], args[2], args[3], args[4], big, None) == -1, miss
        assert b'null buffer' in L.pf_last_error()
    assert L.pf_odom_train_forward(junk, 0, 4, 9, 9, junk, junk, junk, junk, big - 1, None) == -1
    assert b'workspace' in L.pf_last_error()
    for miss in range(5):                                   # packed, inps, out_norm, ws, grad_raw (the grads may be null)
        args = [junk] * 5
        args[miss] = None
        assert L.pf_odom_backward(args[0], 0, 4, 9, 9, args[1], args[2], None, None, args[3], big, args[4], None) == -1, miss
        assert b'null buffer' in L.pf_last_error()
    assert L.pf_odom_backward(junk, 0, 4, 9, 9, junk, junk, junk, junk, junk, big - 1, junk, None) == -1
    assert b'workspace' in L.pf_last_error()
    assert L.pf_odom_backward(None, 0, 0, 9, 9, None, None, None, None, None, 0, None, None) == -1    # B = 0 still writes grad_raw
    assert L.pf_odom_train_forward(None, 0, 0, 9, 9, None, None, None, None, 0, None) == 0     # B = 0: nothing enqueued


def test_train_workspace_grows_with_batch_and_steps():
    L = pflib.load()

    def size(b, t_in, t_out):
        n = ctypes.c_size_t()
        assert L.pf_odom_train_workspace(b, t_in, t_out, 0, ctypes.byref(n)) == 0
        return n.value
    assert size(0, 9, 9) == 0
    assert size(1, 9, 9) >= 17 * 5 * 128 * 4
    assert size(1, 9, 9) < size(32, 9, 9) < size(33, 9, 9) < size(1000, 9, 9) < size(12000, 9, 9)
    assert size(32, 9, 9) < size(32, 10, 9) < size(32, 10, 10) < size(32, 64, 64)
    assert size(1000, 9, 9) >= 1000 * 17 * 5 * 128 * 4
    assert size(32, 9, 9) == size(32, 9, 9) and size(32, 9, 9) % 256 == 0


def test_loss_on_a_host_model_is_not_implemented():
    m = OdomModel(R.odom_params())
    with pytest.raises(NotImplementedError):
        m.loss({'odometry': R.make_inputs(0, 4)}, {'odometry': T.make_labels(0, 4)})
    with pytest.raises(NotImplementedError):
        m.loss({}, {})                                      # the parameters' device is checked before anything is read


def test_optimizer_selection_follows_the_reference():
    m = OdomModel(R.odom_params())
    pick = lambda **tr: type(train_odom.build_optimizer(m, dict(lr=1e-3, **tr)))
    assert pick() is torch.optim.SGD and pick(use_adam=True) is torch.optim.Adam
    assert pick(use_adamw=True) is torch.optim.SGD          # train.py:129-136: the else of use_adam replaces it
    opt = train_odom.build_optimizer(m, dict(lr=1e-3, use_adam=True))
    assert sum(p.numel() for g in opt.param_groups for p in g['params']) == 50946
