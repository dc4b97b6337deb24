"""fg training, host side (no GPU): the float64 checker of tests/fg_train_ref.py pinned to the reference's own float64 ``loss``
and gradients (tests/golden/g11_fgtrain.npz), and the fixture's inputs.  ``FGModel.loss`` itself is not built: this is
the yardstick a native fg training step will be measured against."""
import hashlib
import os

import numpy as np
import pytest
import torch

import fg_ref64 as R
import fg_train_ref as T
from panoptic_forecasting_amd.fg_model import FGModel


@pytest.fixture(scope='module')
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, 'g11_fgtrain.npz'))


@pytest.fixture(scope='module')
def checker():
    """(losses, grads) of loss64 in float64 on the fixture's batch - computed once."""
    sd = R.fill_weights(FGModel(R.fg_params()).state_dict())
    inputs, labels = T.make_batch(0, [3, 2])
    return T.loss_and_grads(sd, inputs, labels)


def test_loss64_reproduces_the_references_float64_loss(fx, checker):
    assert sorted(k[7:] for k in fx.files if k.startswith('loss64_')) == sorted(T.LOSS_KEYS)
    for k in T.LOSS_KEYS:
        ref = torch.from_numpy(fx['loss64_' + k])
        err = (checker[0][k] - ref).abs().max().item()
        print('%-20s err %.3e of max %.4g' % (k, err, ref.abs().max()))
        assert checker[0][k].shape == (5,) and err <= 1e-9 * ref.abs().max().item(), k


def test_loss64_gradients_reproduce_the_references(fx, checker):
    keys = list(fx['keys'])
    assert keys == list(FGModel(R.fg_params()).state_dict().keys())
    seen = 0
    for i, k in enumerate(keys):
        g = checker[1][k]
        if g is None:
            continue
        g = g.reshape(-1).numpy()
        ref = fx['g64_%d' % i] if 'g64_%d' % i in fx else fx['gval_%d' % i]
        got = g if 'g64_%d' % i in fx else g[T.sample_index(i, g.size)]
        big = float(fx['gmax_%d' % i])
        err = np.abs(got - ref).max()
        print('%-45s err/max %.3e' % (k, err / big))
        assert err <= 1e-9 * big, k
        seen += 1
    assert seen == 34


def test_the_same_keys_get_no_gradient(fx, checker):
    none = [k for k, g in checker[1].items() if g is None]
    assert sorted(none) == sorted(fx['none_keys']) and len(none) == 18
    assert sorted(none) == sorted(k for k in fx['keys'] if not T.is_trained(k))


def test_fixture_batch_is_rebuilt_bit_for_bit():
    a_in, a_lab = T.make_batch(0, [3, 2])
    b_in, b_lab = T.make_batch(0, [3, 2])
    for a, b in ((a_in, b_in), (a_lab, b_lab)):
        assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert a_in['feat_masks'].shape == (5, 6) and a_in['bbox_masks'].shape == (5, 6) and a_lab['feats'].shape == (5, 3, 256, 14, 14)
    fm, bm = a_in['feat_masks'], a_in['bbox_masks']
    assert fm[1, 0] == 0 and fm[3, 2] == 0 and fm[2, 4] == 0 and fm.sum() == 27
    assert not bm[2, 5] and not bm[1, 0] and not bm[3, 2] and bm.sum() == 27
    assert not a_lab['depth_masks'][0, 2, 0] and a_lab['depth_masks'].sum() == 14
    # counter-based streams: the same bytes on every machine
    digest = hashlib.sha256(a_lab['trajectories'].numpy().tobytes() + a_lab['feats'].numpy()[:, :, :2].tobytes()).hexdigest()
    assert digest == FIXTURE_DIGEST, digest


FIXTURE_DIGEST = '81eb76f26513d29ecb98f4a8bd5800ff2a68ec911fbe76929631914c9c7adced'
