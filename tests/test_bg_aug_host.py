"""Host side of the bg training augmentation (bg_augment.py, bg_dataset.py): the index tables against the installed Pillow and
against fixture G12 (the reference's own transforms, tests/golden/make_golden_bgaug.py), the random draws, the sample
enumeration and the refusal to compute depth norm parameters.  No GPU."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN

from panoptic_forecasting_amd import bg_augment as A


@pytest.fixture(scope='module')
def g12():
    z = np.load(os.path.join(GOLDEN, 'g12_bgaug.npz'))
    return [{k[len('c%d_' % i):]: z[k] for k in z.files if k.startswith('c%d_' % i)} for i in range(int(z['n_cases']))]


def case_tables(c):
    h, w = c['src_label'].shape
    params = A.draw_params(random.Random(int(c['seed'])), w, h, int(c['size']), float(c['scale_min']), float(c['scale_max']))
    return params, A.build_tables(params, w, h, int(c['size']))


@pytest.mark.parametrize('crop,size', [(c, 40) for c in range(20, 81)] + [(448, 800), (512, 800), (1024, 800)])
def test_label_table_equals_pil_nearest(crop, size):
    """Both axes at once: a ``crop x crop`` image whose pixel (y, x) holds (y + 3 x) mod 251 resized by PIL, against the numpy
    gather through the tables of an unpadded, uncropped, unflipped sample."""
    y, x = np.mgrid[0:crop, 0:crop]
    src = ((y + 3 * x) % 251).astype(np.uint8)
    want = np.array(Image.fromarray(src).resize((size, size), Image.NEAREST))
    params = {'crop_w': crop, 'crop_h': crop, 'pad_w': 0, 'pad_h': 0, 'x1': 0, 'y1': 0, 'flip': False}
    y_map, x_map, _, _ = A.build_tables(params, crop, crop, size)
    assert y_map.dtype == np.int32 and y_map.shape == (size,) and x_map.shape == (size,)
    assert np.array_equal(A.gather_numpy(src, y_map, x_map, 255), want)


def test_the_closed_form_is_not_pils_rule():
    """Why the tables accumulate: floor((x + 0.5) * a) differs from Pillow at the extents the issue names."""
    for crop, size in ((448, 800), (512, 800), (1152, 800), (32, 40), (48, 40), (64, 40)):
        closed = np.floor((np.arange(size) + 0.5) * (crop / size)).astype(np.int64)
        src = (np.arange(crop) % 251).astype(np.uint8)[None].repeat(2, 0)
        pil = np.array(Image.fromarray(src).resize((size, 2), Image.NEAREST))[0]
        assert np.array_equal(src[0][A.pil_nearest_index(crop, size)], pil)
        assert not np.array_equal(src[0][closed], pil), (crop, size)


def test_draw_params_reproduces_the_recorded_draws(g12):
    kinds = set()
    for c in g12:
        params, _ = case_tables(c)
        assert params['scale'] == float(c['scale'])
        assert params['x1'] == max(int(c['x1']), 0) and params['y1'] == max(int(c['y1']), 0)
        assert params['flip'] == bool(c['flip'])
        # a draw the reference skipped (x1 / y1 recorded as -1) is skipped here too: the flip would otherwise differ; and directly:
        h, w = c['src_label'].shape
        assert (int(c['x1']) < 0) == (w + 2 * params['pad_w'] == params['crop_w'])
        assert (int(c['y1']) < 0) == (h + 2 * params['pad_h'] == params['crop_h'])
        kinds.add((params['pad_w'] > 0, params['pad_h'] > 0, params['flip']))
    assert {k[:2] for k in kinds} == {(False, False), (False, True), (True, True)} and {k[2] for k in kinds} == {True, False}


def test_tables_reproduce_the_fixture_planes(g12):
    for i, c in enumerate(g12):
        _, (y_map, x_map, y_arr, x_arr) = case_tables(c)
        assert np.array_equal(A.gather_numpy(c['src_seg'], y_map, x_map, 255), c['out_seg']), i
        assert np.array_equal(A.gather_numpy(c['src_label'], y_map, x_map, 255), c['out_label']), i
        assert np.array_equal(A.gather_numpy(c['src_depth'], y_arr, x_arr, 0), c['out_depth']), i


def test_identity_and_flip_only_tables():
    y_map, x_map, y_arr, x_arr = A.build_tables(None, 7, 5, None)
    assert y_map.tolist() == y_arr.tolist() == list(range(5)) and x_map.tolist() == x_arr.tolist() == list(range(7))
    rng = random.Random(3)
    want = rng.random() < 0.5
    p = A.draw_flip(random.Random(3))
    assert p == {'flip': want}
    _, x_map, _, x_arr = A.build_tables({'flip': True}, 7, 5, None)
    assert x_map.tolist() == x_arr.tolist() == list(range(6, -1, -1))


# ---------------------------------------------------------------------------------------------- dataset
def make_tree(root, frames, h=8, w=12, depth_png=True, groups=1):
    """A tiny exported tree: gt/<split>/<city>/*_labelTrainIds.png and 3 * groups data dirs with label (and depth) PNGs."""
    dirs = [os.path.join(root, 'in%d' % i) for i in range(3 * groups)]
    g = np.random.RandomState(0)
    for split, city, seq, frame in frames:
        os.makedirs(os.path.join(root, 'gt', split, city), exist_ok=True)
        Image.fromarray(g.randint(0, 19, (h, w)).astype(np.uint8)).save(
            os.path.join(root, 'gt', split, city, '%s_%s_%06d_gtFine_labelTrainIds.png' % (city, seq, frame)))
        for d in dirs:
            os.makedirs(os.path.join(d, split, city), exist_ok=True)
            Image.fromarray(g.randint(0, 19, (h, w)).astype(np.uint8)).save(
                os.path.join(d, split, city, '%s_%s_%06d_gtFine_labelIds.png' % (city, seq, frame)))
            if depth_png:
                Image.fromarray(g.randint(0, 65536, (h, w)).astype(np.uint16)).save(
                    os.path.join(d, split, city, '%s_%s_%06d_depths.png' % (city, seq, frame)))
    return dirs


FRAMES = [('train', 'ulm', '000002', 19), ('train', 'aachen', '000010', 49), ('train', 'aachen', '000001', 19),
          ('val', 'bonn', '000004', 19)]


def tree_params(root, dirs, gap_len=(3,), **data):
    d = {'data_dir': dirs, 'gt_dir': os.path.join(root, 'gt'), 'cityscapes_dir': root, 'data_splits': ['train', 'val'],
         'use_depths': True, 'depth_h5_path': os.path.join(root, 'depth_%s.h5'), 'min_depth': 0.1, 'max_depth': 200,
         'only_background': True, 'crop_size': 8, 'scale_min': 0.5, 'scale_max': 2.0, 'gap_len': list(gap_len),
         'depth_norm_params': [20.0, 15.0]}
    d.update(data)
    return {'data': d, 'training': {'batch_size': 2}, 'seed': 1}


def test_enumeration_of_a_tiny_tree(tmp_path):
    from panoptic_forecasting_amd import bg_dataset as D
    root = str(tmp_path)
    dirs = make_tree(root, FRAMES, groups=2)
    params = tree_params(root, dirs, gap_len=(3, 9))
    ds = D.build_dataset(params)
    assert params['data']['num_classes'] == 11 and params['data']['depth_norm_params'] == [20.0, 15.0]
    tr, va = ds['train'], ds['val']
    assert len(tr) == 6 and len(va) == 2 and tr.T == 3
    # sorted by city then file name; per ground-truth frame one entry per (group of 3 dirs, gap_len), start_fr = (9 - gap) / 3
    assert [(s['city'], s['seq'], s['frame'], s['start_fr']) for s in tr.samples] == [
        ('aachen', '000001', 19, 2.0), ('aachen', '000001', 19, 0.0), ('aachen', '000010', 49, 2.0), ('aachen', '000010', 49, 0.0),
        ('ulm', '000002', 19, 2.0), ('ulm', '000002', 19, 0.0)]
    s = tr.samples[3]
    assert s['gt_file'] == os.path.join(root, 'gt', 'train', 'aachen', 'aachen_000010_000049_gtFine_labelTrainIds.png')
    assert s['data_files'] == [os.path.join(d, 'train', 'aachen', 'aachen_000010_000049_gtFine_labelIds.png') for d in dirs[3:]]
    assert s['depth_files'] == [os.path.join(d, 'train', 'aachen', 'aachen_000010_000049_depths.png') for d in dirs[3:]]
    assert tr.source_shape() == (8, 12) and tr.out_shape() == (8, 8) and va.out_shape() == (8, 12)
    # decode: one task per file, each writes its plane
    seg, lab, dep = np.zeros((3, 8, 12), np.uint8), np.zeros((8, 12), np.uint8), np.zeros((3, 8, 12), np.uint16)
    tasks = tr.decode_tasks(3, seg, lab, dep)
    assert len(tasks) == 7
    for t in tasks:
        t()
    assert np.array_equal(lab, np.array(Image.open(s['gt_file'])))
    assert np.array_equal(seg[2], np.array(Image.open(s['data_files'][2])))
    assert np.array_equal(dep[1], np.array(Image.open(s['depth_files'][1])).astype(np.uint16))
    # a sample's parameters depend on (seed, epoch, index) alone; validation has none
    assert tr.draw(1, 2, 3) == tr.draw(1, 2, 3) and tr.draw(1, 2, 3) != tr.draw(1, 3, 3) and va.draw(1, 2, 0) is None
    os.remove(s['data_files'][0])
    with pytest.raises(IOError, match='Could not find data file'):
        D.NativeBGDataset('train', params)


def test_batch_order_shards_and_cycles(tmp_path):
    from panoptic_forecasting_amd import bg_dataset as D
    root = str(tmp_path)
    frames = [('train', 'ulm', '%06d' % i, 19) for i in range(7)] + [('val', 'bonn', '%06d' % i, 19) for i in range(3)]
    dirs = make_tree(root, frames, depth_png=False)
    params = tree_params(root, dirs, use_depths=False)
    ds = D.build_dataset(params)
    one = D.NativeBatches(ds['train'], params, 0, 1, train=True)
    b = one.index_batches(5)
    assert len(one) == 3 and [len(x) for x in b] == [2, 2, 2] and len({i for x in b for i in x}) == 6     # drop_last
    assert b == one.index_batches(5) and b != one.index_batches(6)
    halves = [D.NativeBatches(ds['train'], params, r, 2, train=True).index_batches(5) for r in (0, 1)]
    flat = [i for h in halves for x in h for i in x]
    assert [len(h) for h in halves] == [1, 1] and len(set(flat)) == 4                                      # disjoint strided shards
    params['training']['steps_per_epoch'] = 4
    params['training']['accumulate_steps'] = 2
    cyc = D.NativeBatches(ds['train'], params, 0, 1, train=True)
    assert len(cyc) == 8 and len(cyc.index_batches(1)) == 8 and cyc.index_batches(1)[:3] != cyc.index_batches(1)[3:6]
    val = D.NativeBatches(ds['val'], params, 0, 1, train=False)
    assert val.index_batches(1) == [[0, 1], [2]] and len(val) == 2
    assert D.NativeBatches(ds['val'], params, 1, 2, train=False).index_batches(1) == [[1]]
    params['training']['num_data_workers'] = 64
    assert D.NativeBatches(ds['train'], params, 0, 1, train=True).threads == 16


def test_missing_norm_file_raises_the_named_error(tmp_path):
    from panoptic_forecasting_amd import bg_dataset as D
    root = str(tmp_path)
    dirs = make_tree(root, FRAMES)
    params = tree_params(root, dirs, depth_norm_params=None, depth_norm_params_file=os.path.join(root, 'norm.pt'))
    with pytest.raises(D.BGDatasetError, match=r'data\.depth_norm_params_file'):
        D.build_dataset(params)
    torch.save([torch.FloatTensor([21.5]), torch.FloatTensor([14.25])], os.path.join(root, 'norm.pt'))   # as bg_dataset.py:133-136 saves it
    D.build_dataset(params)
    assert params['data']['depth_norm_params'] == [21.5, 14.25]
    with pytest.raises(D.BGDatasetError, match='resize_w'):
        D.NativeBGDataset('train', tree_params(root, dirs, resize_w=16, resize_h=8))
