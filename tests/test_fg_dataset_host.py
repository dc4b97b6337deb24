"""The native fg scene dataset on the host: enumeration + ``assemble_host`` against the reference's own ``FGSceneDataset`` and
``collate_fn`` (tests/golden/g13_fgscene.npz, G13), the pkl and npz routes, the refused keys, and the missing-file pass of the
panoptic export.  No GPU: ``pf_fg_assemble`` is held to the same fixture in tests/test_gpu_fg_dataset.py."""
import json
import os

import numpy as np
import pytest
import torch

import fgscene_tree as FT

CONFIGS = ('mid', 'short', 'gap', 'gap_short', 'ulbr')


@pytest.fixture(scope='module')
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, 'g13_fgscene.npz'))


@pytest.fixture(scope='module')
def tree(fx, tmp_path_factory):
    root = str(tmp_path_factory.mktemp('g13'))
    FT.write_g13(root, fx)
    return root


def _dataset(fx, root, name, **data_overrides):
    from panoptic_forecasting_amd import fg_dataset as D
    params = FT.g13_params(FT.g13_configs(fx)[name], root)
    params['data'].update(data_overrides)
    return D.NativeFGSceneDataset(FT.SPLIT, params, test=True), params


@pytest.mark.parametrize('name', CONFIGS)
def test_host_batch_reproduces_the_reference(fx, tree, name):
    ds, params = _dataset(fx, tree, name)
    assert len(ds) == 4
    assert params['data']['num_classes'] == 19 and params['data']['odom_size'] == 5
    assert torch.equal(params['data']['img_size'], torch.tensor([2048., 1024.]))
    batch = ds.host_batch(range(len(ds)))
    FT.check_batch_against_g13(fx, name, batch)
    assert [len(c) for c in batch['inputs']['classes']][2] == 0
    assert 'feats' not in batch['labels']
    # batches of two scenes hold the same per-scene tensors
    for start in (0, 2):
        part = ds.host_batch(range(start, start + 2))
        for group in ('inputs', 'labels'):
            for field, vals in part[group].items():
                for j, v in enumerate(vals):
                    assert torch.equal(v, batch[group][field][start + j]), (group, field, start + j)


def test_the_fixture_holds_the_cases_it_is_for(fx):
    """The car-gap filter fired, depths of every excluded kind occur, an observed step has no feature row."""
    mid, gap = 'out.mid.inputs.%s.0', 'out.gap.inputs.%s.0'
    assert fx[mid % 'bbox_masks'][0].sum() > fx[gap % 'bbox_masks'][0].sum()
    assert (fx[gap % 'trajectories'][0, 2] == 0).all() and (fx[mid % 'trajectories'][0, 2] != 0).any()
    assert not np.array_equal(fx['out.ulbr.inputs.bbox_masks.0'][1], np.ones(6, bool))          # the right-border car, ulbr reading only
    assert np.array_equal(fx[gap % 'bbox_masks'][1], np.ones(6, bool))
    d = fx['in.cascade.0']
    assert (d == -1).any() and (d == 1000000).any() and (d > 200).any()
    assert not fx[gap % 'depth_masks'].all() and fx[mid % 'depth_masks'].sum() > fx[gap % 'depth_masks'].sum()
    assert ((fx['in.condensed.0'] == -1) & fx['in.meta.feat_mask.0']).any()
    assert fx['out.short.meta.fr_inds.0'].tolist() == [10, 13, 16, 19, 22, 25] and int(fx['out.short.meta.target_frame.1']) == 25


def test_pkl_and_npz_routes_agree(fx, tree, tmp_path):
    pytest.importorskip('pandas')
    from panoptic_forecasting_amd import fg_dataset as D
    root = str(tmp_path / 'pkl')
    FT.write_g13(root, fx, as_pkl=True)
    assert os.path.exists(os.path.join(root, 'val_seq_meta.pkl')) and not os.path.exists(os.path.join(root, 'val_seq_meta.npz'))
    a = _dataset(fx, root, 'gap')[0].host_batch(range(4))
    b = _dataset(fx, tree, 'gap')[0].host_batch(range(4))
    for group in ('inputs', 'labels'):
        for field in a[group]:
            for x, y in zip(a[group][field], b[group][field]):
                assert x.dtype == y.dtype and torch.equal(x, y), (group, field)
    # the converter writes the twin the loader reads
    twin = D.convert_to_npz(os.path.join(root, 'val_seq_meta.pkl'), str(tmp_path / 'meta_twin.npz'))
    t, want = D.read_table(twin), D.read_table(os.path.join(tree, 'val_seq_meta.npz'))
    for col in FT.META_COLS + ('city', 'seq', 'frame'):
        for x, y in zip(t[col], want[col]):
            assert np.array_equal(x, y), col


def test_a_missing_file_says_how_to_convert(fx, tree, tmp_path):
    from panoptic_forecasting_amd import fg_dataset as D
    params = FT.g13_params(FT.g13_configs(fx)['mid'], tree)
    params['data']['depth_dir'] = str(tmp_path)
    with pytest.raises(D.FGDatasetError, match='convert_to_npz'):
        D.NativeFGSceneDataset(FT.SPLIT, params, test=True)


@pytest.mark.parametrize('key,value', [('expand_test', True), ('use_orbslam_odom', True), ('no_feats', True), ('input_len', 4)])
def test_refused_keys_name_themselves(fx, tree, key, value):
    from panoptic_forecasting_amd import fg_dataset as D
    with pytest.raises(D.FGDatasetError, match='data.' + key):
        _dataset(fx, tree, 'mid', **{key: value})


def test_training_path_is_refused(fx, tree):
    from panoptic_forecasting_amd import fg_dataset as D
    params = FT.g13_params(FT.g13_configs(fx)['mid'], tree)
    with pytest.raises(D.FGDatasetError, match='test=False'):
        D.NativeFGSceneDataset(FT.SPLIT, params, test=False)
    with pytest.raises(D.FGDatasetError, match='train'):
        D.NativeFGSceneDataset('train', params, test=True)


@pytest.mark.parametrize('bad', [4, -2])
def test_out_of_range_feat_ind_raises(fx, tmp_path, bad):
    from panoptic_forecasting_amd import fg_dataset as D
    root = str(tmp_path / 'bad')
    FT.write_g13(root, fx)
    path = os.path.join(root, 'val_seq_condensed_feat_info.npz')
    arrs = dict(np.load(path))
    rows = arrs['feat_ind__rows']
    assert arrs['feat_ind'][rows[0], 10] >= 0           # scene 1, instance 0, the most recent input step of the mid window
    arrs['feat_ind'][rows[0], 10] = bad
    np.savez_compressed(path, **arrs)
    ds, _ = _dataset(fx, root, 'mid')
    ds.host_batch([0])
    with pytest.raises(D.FGDatasetError, match='feat_ind %d' % bad):
        ds.host_batch([1])


def test_assemble_host_guards_feat_row_like_the_kernel():
    from panoptic_forecasting_amd import fg_dataset as D
    t = {k: torch.from_numpy(v) for k, v in FT.random_tables(5, 3, seed=1).items()}
    t['feat_row'][0, 0], t['feat_row'][1, 1], t['feat_row'][2, 2] = 3, -7, 2
    out = D.assemble_host(**t, filter_car_gap=20, max_depth=200)
    assert not out['feats'][0, 0].any() and not out['feats'][1, 1].any() and torch.equal(out['feats'][2, 2], t['feat_table'][2])
    assert out['feats'].shape == (5, 3, 256, 14, 14) and out['trajectories'].shape == (5, 6, 8)
    empty = D.assemble_host(**{k: torch.from_numpy(v) for k, v in FT.random_tables(0, 0, seed=1).items()})
    assert empty['feats'].shape == (0, 3, 256, 14, 14) and empty['one_hot_classes'].shape == (0, 8)


def test_fill_missing_panoptic(tmp_path):
    """A prediction present (left alone), only a background present (converted and encoded, whatever --no_convert said), neither
    (all zero, no segments); an empty ground-truth folder is not an error."""
    from PIL import Image
    from panoptic_forecasting_amd import panoptic as pp
    gt = tmp_path / 'gtFine' / 'val'
    (gt / 'ulm').mkdir(parents=True)
    (gt / 'bonn').mkdir()
    bgd = tmp_path / 'bg' / 'val'
    (bgd / 'ulm').mkdir(parents=True)
    for stem in ('ulm_000001_000019', 'ulm_000002_000019', 'ulm_000003_000019'):
        Image.fromarray(np.zeros((4, 8), np.uint8)).save(str(gt / 'ulm' / (stem + '_gtFine_labelIds.png')))
    seg_dir = tmp_path / 'out' / 'pan_val'
    seg_dir.mkdir(parents=True)
    kept = np.full((4, 8, 3), 9, np.uint8)
    Image.fromarray(kept).save(str(seg_dir / 'ulm_000001_000019_pred_panoptic.png'))
    bg = np.array([[0, 0, 1, 1, 10, 10, 255, 255], [13, 13, 13, 11, 11, 18, 18, 255]] * 2, np.uint8)
    Image.fromarray(bg).save(str(bgd / 'ulm' / 'ulm_000002_000019_gtFine_labelIds.png'))
    ann = [{'file_name': 'ulm_000001_000019_pred_panoptic.png', 'image_id': 'ulm_000001_000019', 'segments_info': []}]
    n = pp.fill_missing_panoptic(str(tmp_path / 'out'), 'pan_val', str(gt), background_dir=str(bgd), annotations=ann)
    assert n == 2 and [a['image_id'] for a in ann] == ['ulm_000001_000019', 'ulm_000002_000019', 'ulm_000003_000019']
    assert np.array_equal(np.array(Image.open(str(seg_dir / 'ulm_000001_000019_pred_panoptic.png'))), kept)
    ids = pp.decode_png(np.array(Image.open(str(seg_dir / 'ulm_000002_000019_pred_panoptic.png'))))
    lut = np.zeros(256, np.int64)
    lut[:19] = pp.TRAINID2ID
    assert np.array_equal(ids, lut[bg])
    assert ann[1]['file_name'] == 'ulm_000002_000019_pred_panoptic.png'
    assert ann[1]['segments_info'] == [{'category_id': v, 'id': v} for v in (7, 8, 23, 24, 26, 33)]
    zero = np.array(Image.open(str(seg_dir / 'ulm_000003_000019_pred_panoptic.png')))
    assert zero.shape == (1024, 2048, 3) and not zero.any() and ann[2]['segments_info'] == []
    json.dumps(ann)
    # nothing to do the second time; and a ground-truth folder without a single city or frame only reports
    assert pp.fill_missing_panoptic(str(tmp_path / 'out'), 'pan_val', str(gt), background_dir=str(bgd)) == 0
    (tmp_path / 'empty').mkdir()
    assert pp.fill_missing_panoptic(str(tmp_path / 'out'), 'pan_val', str(tmp_path / 'empty'), background_dir=None) == 0
