"""``pf_fg_assemble`` and the native fg loader on the MI355X: the kernel against the reference's recorded batches (G13) and against
``assemble_host`` bit for bit, its guard on ``feat_row``, a captured launch replayed, and the export driver end to end."""
import json
import os

import numpy as np
import pytest
import torch

import fg_ref64 as R
import fgscene_tree as FT

pytestmark = pytest.mark.gpu
REPLAYS = 5
FLOATS = ('trajectories', 'depths', 'one_hot_classes', 'final_bboxes', 'feats')
# (use_ulbr, max_depth, filter_car_gap): the shipped configuration, the filter in both readings, a gap that is no fp32 number
MODES = [(False, None, None), (False, 200, 20), (True, 200.5, 20.1)]


@pytest.fixture(scope='module')
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, 'g13_fgscene.npz'))


@pytest.fixture(scope='module')
def tree(fx, tmp_path_factory):
    root = str(tmp_path_factory.mktemp('g13'))
    FT.write_g13(root, fx)
    return root


def _same_bits(got, want, what):
    assert set(got) == set(want)
    for k in want:
        g, w = got[k].cpu(), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if k in FLOATS:
            g, w = g.contiguous().view(torch.int32), w.contiguous().view(torch.int32)
        assert torch.equal(g, w), (what, k, int((g != w).sum()))


def _on_device(tables):
    return {k: torch.from_numpy(v).cuda() for k, v in tables.items()}


@pytest.mark.parametrize('name', ['mid', 'short', 'gap', 'gap_short', 'ulbr'])
def test_device_batch_equals_the_reference(fx, tree, name):
    from panoptic_forecasting_amd import fg_dataset as D
    ds = D.NativeFGSceneDataset(FT.SPLIT, FT.g13_params(FT.g13_configs(fx)[name], tree), test=True)
    batch = ds.device_batch(range(len(ds)))
    assert all(v.is_cuda for vals in batch['inputs'].values() for v in vals)
    FT.check_batch_against_g13(fx, name, batch)
    two = list(ds.batches(2))                       # the loader's own batching: staging buffers reused between batches
    assert len(two) == 2
    for b, part in enumerate(two):
        for group in ('inputs', 'labels'):
            for field, vals in part[group].items():
                for j, v in enumerate(vals):
                    assert torch.equal(v, batch[group][field][2 * b + j]), (group, field, 2 * b + j)
    ds.close()


@pytest.fixture(scope='module')
def host_results():
    """assemble_host of every (n, mode), computed once."""
    from panoptic_forecasting_amd import fg_dataset as D
    out = {}
    for n in (0, 1, 5, 257):
        tables = FT.random_tables(n, 0 if n == 0 else 16, seed=40 + n)
        for mi, (ulbr, max_depth, gap) in enumerate(MODES):
            out[n, mi] = (tables, D.assemble_host(**{k: torch.from_numpy(v) for k, v in tables.items()}, use_ulbr=ulbr,
                                                  max_depth=max_depth, filter_car_gap=gap))
    return out


@pytest.mark.parametrize('mi', range(len(MODES)))
@pytest.mark.parametrize('n', [0, 1, 5, 257])
def test_kernel_equals_assemble_host(host_results, n, mi):
    """N = 257 is past one 256-lane workgroup of the per-instance part (and 5 397 gather workgroups)."""
    from panoptic_forecasting_amd import fg_dataset as D
    tables, want = host_results[n, mi]
    ulbr, max_depth, gap = MODES[mi]
    got = D.device_assemble(**_on_device(tables), use_ulbr=ulbr, max_depth=max_depth, filter_car_gap=gap)
    torch.cuda.synchronize()
    _same_bits(got, want, (n, mi))
    if n == 257 and gap is not None:                # the filter fired in these tables (43 cars at the left border)
        assert not torch.equal(want['bbox_masks'], torch.from_numpy(tables['feat_mask']).bool())


def test_out_of_range_feat_row_gives_zeros():
    from panoptic_forecasting_amd import fg_dataset as D
    tables = FT.random_tables(5, 3, seed=7)
    tables['feat_row'][:] = [[0, 3, -1], [2, 2 ** 31 - 1, -2 ** 31], [1000000, 1, -5], [3, 4, 2], [-1, -1, -1]]
    got = D.device_assemble(**_on_device(tables), filter_car_gap=20, max_depth=200)
    torch.cuda.synchronize()
    want = D.assemble_host(**{k: torch.from_numpy(v) for k, v in tables.items()}, filter_car_gap=20, max_depth=200)
    _same_bits(got, want, 'guard')
    feats = got['feats'].cpu()
    table = torch.from_numpy(tables['feat_table'])
    for (i, t), row in {(0, 0): 0, (1, 0): 2, (2, 1): 1, (3, 2): 2}.items():
        assert torch.equal(feats[i, t], table[row])
    for i, t in ((0, 1), (0, 2), (1, 1), (1, 2), (2, 0), (2, 2), (3, 0), (3, 1), (4, 0), (4, 1), (4, 2)):
        assert not feats[i, t].any(), (i, t)


def test_captured_launch_replays_equal_eager():
    """One kernel node: captured once, replayed five times over outputs that were overwritten in between."""
    from panoptic_forecasting_amd import fg_dataset as D
    dev = _on_device(FT.random_tables(37, 8, seed=3))
    kw = dict(use_ulbr=False, max_depth=200, filter_car_gap=20)
    want = {k: v.clone() for k, v in D.device_assemble(**dev, **kw).items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = D.device_assemble(**dev, **kw)
    for rep in range(REPLAYS):
        for v in out.values():
            (v.view(torch.uint8) if v.dtype == torch.bool else v).fill_(77)
        g.replay()
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(out[k], want[k]), (rep, k)


def test_export_panoptic_end_to_end(tmp_path):
    """odometry / bg export files on disk -> export_panoptic.main -> PNGs + JSON -> eval_panoptic, with no reference code: the PNGs
    decode to what predict_panoptic gives for the same batch assembled by assemble_host (same inputs, same kernels: exact)."""
    import yaml
    from PIL import Image
    from oracle import panoptic as op
    from panoptic_forecasting_amd import eval_panoptic, export_panoptic, fg_dataset as D, panoptic as pp
    from panoptic_forecasting_amd.registry import build_model
    root = str(tmp_path / 'data')
    scenes, data = FT.write_synthetic(root, n_scenes=2, seed=5)
    cs = tmp_path / 'cityscapes'
    gt_dir = cs / 'gtFine' / FT.SPLIT / 'synth'
    gt_dir.mkdir(parents=True)
    for seq in ('000001', '000002', '000009'):      # the third frame has neither a prediction nor a background
        (gt_dir / ('synth_%s_000019_gtFine_labelIds.png' % seq)).write_bytes(b'')
    data['cityscapes_dir'] = str(cs)
    config = {'task': 'fg', 'model': dict(R.FG_CONFIG, use_depth_sorting=True), 'data': data, 'training': {'batch_size': 2}}
    ckpt_dir = tmp_path / 'ckpt'
    ckpt_dir.mkdir()
    with open(str(ckpt_dir / 'config.yaml'), 'w') as f:
        yaml.safe_dump(config, f)
    params = R.fg_params(use_depth_sorting=True)
    params['no_gpu'] = False
    model = build_model(params)
    model.load_state_dict(R.fill_weights(model.state_dict()))
    model.save(str(ckpt_dir / 'fg_model.pt'))

    out = export_panoptic.main(['--config_file', str(ckpt_dir / 'config.yaml'), '--load_model', str(ckpt_dir / 'fg_model.pt'),
                                '--export_name', 'pan', '--working_dir', str(tmp_path / 'work')])
    result_dir, ann_file, n_ann = out[FT.SPLIT]
    assert result_dir == os.path.join(str(tmp_path / 'work'), 'pan_val') and ann_file == os.path.join(result_dir, 'pan_val.json')
    rec = json.load(open(ann_file))['annotations']
    assert n_ann == 3 and [r['image_id'] for r in rec] == ['synth_000001_000019', 'synth_000002_000019', 'synth_000009_000019']
    assert [r['file_name'] for r in rec] == [r['image_id'] + '_pred_panoptic.png' for r in rec]
    assert sorted(os.listdir(os.path.join(result_dir, 'pan_val'))) == sorted(r['file_name'] for r in rec)
    assert rec[2]['segments_info'] == []

    ds = D.NativeFGSceneDataset(FT.SPLIT, {'data': dict(data)}, test=True)
    host = ds.host_batch(range(2))
    assert sum(len(c) for c in host['inputs']['classes']) >= 6
    with torch.no_grad():
        seg = model.predict_panoptic(host['inputs'], host['labels'])['seg']
    assert (seg >= 11000).any() and (seg < 11).any()
    for b in range(2):
        ids = pp.decode_png(np.array(Image.open(os.path.join(result_dir, 'pan_val', rec[b]['file_name']))))
        _, want_ids, present = op.encode(seg[b].cpu(), convert=True)
        assert ids.shape == (1024, 2048) and np.array_equal(ids, want_ids), b
        assert [s['id'] for s in rec[b]['segments_info']] == [i for i in sorted(present) if i != 0]
        assert all(s['category_id'] == (s['id'] // 1000 if s['id'] > 100 else s['id']) for s in rec[b]['segments_info'])

    res = eval_panoptic.run(eval_panoptic.parse_args(['--gt-json-file', ann_file, '--prediction-json-file', ann_file,
                                                      '--results_file', str(tmp_path / 'pq.json')]))
    assert res['All']['n'] > 0 and abs(100 * res['All']['pq'] - 100.0) < 1e-9
    assert json.load(open(str(tmp_path / 'pq.json')))['All']['n'] == res['All']['n']
