"""Semantic IoU on the host: semantic_iou.confusion_host / iou_from_confusion and the drivers eval_semantic.py (host matcher) and
export_semantic.py (naming) against tests/conf_ref64.py.  Tables are integers and must be EQUAL; an IoU is one fp64 division of
two integers below 2^53 (exact operands, one rounding, at most a few ulp apart from the restatement's scale-then-mean order):
1e-12 relative leaves three orders of magnitude."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import conf_ref64 as C
import conf_scenes as CS

REL = 1e-12
V = 255


def host_table(pred, gt, n_cls=19, fmt='trainid'):
    from panoptic_forecasting_amd import semantic_iou as si
    return si.confusion_host(torch.from_numpy(np.asarray(pred)), torch.from_numpy(np.asarray(gt)), n_cls, fmt).numpy()


def table(cells):
    t = np.zeros((20, 20), np.int64)
    for (g, p), n in cells.items():
        t[g, p] = n
    return t


HAND = [
    ('all void', [[V, V, 19], [200, V, 34]], [[V, 30, V], [V, V, 99]], {(19, 19): 6}),
    ('void prediction on valid ground truth', [[V, V], [V, 0]], [[0, 0], [5, 0]], {(0, 19): 2, (5, 19): 1, (0, 0): 1}),
    ('valid prediction on void ground truth', [[3, 3], [18, 3]], [[V, V], [V, 3]], {(19, 3): 2, (19, 18): 1, (3, 3): 1}),
    ('one class only', [[7, 7, 7], [7, 7, 7]], [[7, 7, 7], [7, 7, 7]], {(7, 7): 6}),
]


@pytest.mark.parametrize('name,pred,gt,cells', HAND, ids=[h[0] for h in HAND])
def test_hand_made_maps(name, pred, gt, cells):
    pred, gt = np.array([pred], np.int64), np.array([gt], np.int64)
    want = table(cells)
    ref, per = C.confusion(pred, gt)
    assert np.array_equal(ref, want) and np.array_equal(per[0], want)
    assert np.array_equal(host_table(pred, gt), want)
    assert np.array_equal(host_table(C.to_cityscapes(pred), C.to_cityscapes(gt), fmt='cityscapes'), want)


@pytest.mark.parametrize('fmt', ['trainid', 'cityscapes'])
@pytest.mark.parametrize('n_cls', [1, 11, 19])
def test_random_maps_equal_the_restatement(fmt, n_cls):
    pred, gt = CS.random_maps((3, 37, 61), seed=n_cls, fmt=fmt)
    want, _ = C.confusion(pred, gt, n_cls, fmt)
    assert want.sum() == 3 * 37 * 61 and want[:n_cls, :n_cls].sum() > 0 and want[n_cls:19].sum() == 0 and want[:, n_cls:19].sum() == 0
    for dtype in (torch.uint8, torch.int32, torch.int64):
        from panoptic_forecasting_amd import semantic_iou as si
        got = si.confusion_host(torch.from_numpy(pred).to(dtype), torch.from_numpy(gt).to(dtype), n_cls, fmt)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)


def test_scenes_add_into_acc_and_values_out_of_range_raise():
    from panoptic_forecasting_amd import semantic_iou as si
    pred, gt = CS.make_scenes(n=4)
    want, _ = C.confusion(pred, gt)
    acc = si.confusion_host(torch.from_numpy(pred[:2]), torch.from_numpy(gt[:2]))
    out = si.confusion_host(torch.from_numpy(pred[2:]), torch.from_numpy(gt[2:]), acc=acc)
    assert out is acc and np.array_equal(acc.numpy(), want)
    for bad in (-1, 256, 2 ** 33 + 5):
        p = torch.from_numpy(pred[:1]).clone()
        p[0, 3, 3] = bad
        with pytest.raises(ValueError, match='outside'):
            si.confusion_host(p, torch.from_numpy(gt[:1]))
    with pytest.raises(ValueError):
        si.confusion_host(torch.zeros(1, 2, 2, dtype=torch.uint8), torch.zeros(1, 2, 2, dtype=torch.uint8), fmt='coco')
    with pytest.raises(ValueError):
        si.confusion_host(torch.zeros(1, 2, 2, dtype=torch.uint8), torch.zeros(1, 2, 2, dtype=torch.uint8), n_cls=20)


def assert_iou(got, want):
    for k in ('All', 'Stuff', 'MO'):
        assert got[k]['n'] == want[k]['n'], k
        if want[k]['n']:
            assert abs(got[k]['miou'] - want[k]['miou']) <= REL * abs(want[k]['miou']), k
        else:
            assert math.isnan(got[k]['miou']) and math.isnan(want[k]['miou'])
    assert len(got['per_class']) == len(want['per_class']) == 19
    for c, (a, b) in enumerate(zip(got['per_class'], want['per_class'])):
        assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= REL * abs(b), c
    assert abs(got['pixel_acc'] - want['pixel_acc']) <= REL * abs(want['pixel_acc'])


def test_iou_of_scene_tables_and_of_large_counts():
    from panoptic_forecasting_amd import semantic_iou as si
    pred, gt = CS.make_scenes(n=6)
    t, _ = C.confusion(pred, gt)
    for scale in (100.0, 1.0):
        assert_iou(si.iou_from_confusion(torch.from_numpy(t), scale), C.iou(t, scale))
    rng = np.random.default_rng(3)
    big = rng.integers(0, 2 ** 40, (20, 20))                   # a full validation set's counts and beyond
    assert_iou(si.iou_from_confusion(torch.from_numpy(big)), C.iou(big))


def test_absent_class_is_left_out_and_the_splits_differ():
    """Class 0: tp 6, fn 2 (one of them a void prediction), fp 2 -> 0.6; the prediction on void ground truth is excused.
    Class 12: tp 1, fn 3, fp 1 -> 0.2.  Class 5 only ever appears as a prediction on void ground truth: absent."""
    from panoptic_forecasting_amd import semantic_iou as si
    t = table({(0, 0): 6, (0, 12): 1, (0, 19): 1, (12, 0): 2, (12, 12): 1, (12, 19): 1, (19, 0): 7, (19, 5): 4, (19, 19): 9})
    got = si.iou_from_confusion(torch.from_numpy(t))
    assert got['All']['n'] == 2 and got['Stuff']['n'] == 1 and got['MO']['n'] == 1
    assert got['per_class'][0] == 100.0 * (6 / 10) and got['per_class'][12] == 100.0 * (1 / 5)
    assert math.isnan(got['per_class'][5]) and math.isnan(got['per_class'][18])
    assert got['Stuff']['miou'] == got['per_class'][0] and got['MO']['miou'] == got['per_class'][12]
    assert abs(got['All']['miou'] - 40.0) <= REL * 40.0
    assert len({got['All']['miou'], got['Stuff']['miou'], got['MO']['miou']}) == 3
    assert got['pixel_acc'] == 100.0 * (7 / 12)
    assert_iou(got, C.iou(t))
    empty = si.iou_from_confusion(torch.zeros(20, 20, dtype=torch.int64))
    assert empty['All']['n'] == 0 and math.isnan(empty['All']['miou']) and math.isnan(empty['pixel_acc'])


def test_status_bit_of_the_header_is_the_one_the_meter_names():
    from panoptic_forecasting_amd import semantic_iou as si
    text = open(os.path.join(ROOT, 'include', 'pfhip.h')).read()
    header = {name: int(v) for name, v in re.findall(r'^#define (PF_CONF_STATUS_[A-Z]+) (\d+)u$', text, re.M)}
    assert header == {'PF_CONF_STATUS_VALUE': 1}
    assert {text.split(':')[0]: bit for bit, text in si.STATUS_BITS} == header
    from panoptic_forecasting_amd import lib
    assert lib.load().pf_confusion_chunk_pixels() == 16384
    assert re.search(r'pf_confusion_chunk_pixels\(\) = 16384', text)


@pytest.mark.parametrize('fmt,export_names', [('cityscapes', False), ('trainid', False), ('trainid', True)])
def test_driver_host_matcher_end_to_end(tmp_path, fmt, export_names, capsys):
    from panoptic_forecasting_amd import eval_semantic
    pred, gt = CS.make_scenes(n=3, h=32, w=48, seed=9)
    flags = CS.write_tree(str(tmp_path), pred, gt, fmt, export_names)
    out = str(tmp_path / 'res.json')
    res = eval_semantic.run(eval_semantic.parse_args(flags + ['--results_file', out, '--matcher', 'host', '--batch_size', '2',
                                                              '--num_workers', '2']))
    t, _ = C.confusion(pred, gt)
    want = C.iou(t, scale=1.0)
    with open(out) as f:
        doc = json.load(f)
    assert doc == json.loads(json.dumps(res))
    assert np.array_equal(np.array(doc['confusion']), t)
    nan = lambda x: float('nan') if x is None else x
    assert_iou({'All': {'miou': nan(doc['All']['miou']), 'n': doc['All']['n']}, 'Stuff': {'miou': nan(doc['Stuff']['miou']), 'n': doc['Stuff']['n']},
                'MO': {'miou': nan(doc['MO']['miou']), 'n': doc['MO']['n']}, 'per_class': [nan(x) for x in doc['per_class'].values()],
                'pixel_acc': doc['pixel_acc']}, want)
    assert list(doc['per_class']) == list(eval_semantic.LABEL_NAMES) and doc['All']['n'] > 0
    printed = capsys.readouterr().out
    assert 'road' in printed and 'pixel accuracy' in printed and 'MO' in printed


def test_driver_refusals(tmp_path):
    from PIL import Image
    from panoptic_forecasting_amd import eval_semantic
    pred, gt = CS.make_scenes(n=3, h=32, w=48, seed=9)
    flags = CS.write_tree(str(tmp_path), pred, gt, 'cityscapes') + ['--results_file', str(tmp_path / 'r.json'), '--matcher', 'host']
    victim = os.path.join(str(tmp_path), 'pred', 'city1', 'city1_000001_000019_gtFine_labelIds.png')
    keep = open(victim, 'rb').read()
    os.remove(victim)
    with pytest.raises(eval_semantic.EvalError, match='no prediction for ground-truth image city1.city1_000001_000019_gtFine_labelIds.png'):
        eval_semantic.run(eval_semantic.parse_args(flags))
    Image.fromarray(np.zeros((32, 47), np.uint8)).save(victim)
    with pytest.raises(eval_semantic.EvalError, match='city1_000001.*ground truth is 32x48, prediction 32x47'):
        eval_semantic.run(eval_semantic.parse_args(flags))
    Image.fromarray(np.zeros((32, 48, 3), np.uint8)).save(victim)
    with pytest.raises(eval_semantic.EvalError, match='not an 8-bit single-channel label PNG'):
        eval_semantic.run(eval_semantic.parse_args(flags))
    Image.fromarray(np.zeros((32, 48), np.uint16)).save(victim)
    with pytest.raises(eval_semantic.EvalError, match='not an 8-bit single-channel label PNG'):
        eval_semantic.run(eval_semantic.parse_args(flags))
    open(victim, 'wb').write(keep)
    assert eval_semantic.run(eval_semantic.parse_args(flags))['All']['n'] > 0
    with pytest.raises(eval_semantic.EvalError, match='no ground truth'):
        eval_semantic.run(eval_semantic.parse_args(['--gt-folder', str(tmp_path / 'pred' / 'city0'), '--prediction-folder', str(tmp_path / 'pred')]))
    assert not os.path.exists(os.path.join(ROOT, 'resultPixelLevelSemanticLabeling.json'))


class StubModel:
    """predict_semantics of two fixed frames per batch: class + 11 values over background trainIds, int64 as the merger's."""

    def __init__(self):
        self.calls = 0

    def predict_semantics(self, inputs, labels):
        self.calls += 1
        seg = torch.full((len(inputs['ids']), 8, 16), 255, dtype=torch.int64)
        seg[:, :4] = 2
        seg[:, 4:, :5] = 13
        seg[:, 6:, 10:] = torch.tensor(inputs['ids']).view(-1, 1, 1) % 19
        return {'seg': seg, 'bbox': None, 'depths': None}


class StubDataset:
    split = 'val'
    background_dir = None

    def batches(self, batch_size):
        ids = [1, 2, 7]
        for i in range(0, len(ids), batch_size):
            part = ids[i:i + batch_size]
            yield {'inputs': {'ids': part}, 'labels': {}, 'meta': {'city': ['ulm' if k < 7 else 'bonn' for k in part],
                                                                  'seq': ['%06d' % k for k in part], 'target_frame': [19] * len(part)}}


@pytest.mark.parametrize('no_convert', [False, True])
def test_export_semantic_names_and_modes_with_a_stub_model(tmp_path, monkeypatch, no_convert):
    """The driver's loop, folder and file names and its fill of missing frames; the device conversion is stood in for by its
    definition (trainId -> id, anything else 0; as it is with --no_convert), which tests/test_gpu_hop_io.py checks on the GPU."""
    from panoptic_forecasting_amd import export_semantic, hop_io
    seen = []

    def device_export(seg=None, depth=None, mode=hop_io.SEG_AS_IS):
        seen.append((seg.dtype, mode))
        lut = torch.zeros(256, dtype=torch.uint8)
        lut[:19] = torch.tensor(list(C.ID_OF_TRAINID.values()), dtype=torch.uint8)
        return (lut[seg] if mode == hop_io.SEG_TRAINID_TO_ID else seg.to(torch.uint8)), None

    monkeypatch.setattr(hop_io, 'device_export', device_export)
    gt_dir = tmp_path / 'cs' / 'gtFine' / 'val' / 'ulm'
    gt_dir.mkdir(parents=True)
    for seq in (1, 2, 5):                                  # frame 5 has no prediction
        (gt_dir / ('ulm_%06d_000019_gtFine_labelIds.png' % seq)).write_bytes(b'')
    params = {'working_dir': str(tmp_path / 'work'), 'no_convert': no_convert, 'training': {'batch_size': 2},
              'data': {'cityscapes_dir': str(tmp_path / 'cs')}}
    if not no_convert:
        params['export_name'] = 'sem_mid'
    model = StubModel()
    result_dir, written, missing = export_semantic.export_split(model, StubDataset(), 'val', params)
    assert result_dir == os.path.join(str(tmp_path / 'work'), 'exported_semantics_val' if no_convert else 'sem_mid_val')
    assert model.calls == 2 and missing == 1
    assert seen == [(torch.int64, hop_io.seg_mode(no_convert))] * 2
    assert [os.path.relpath(p, result_dir) for p in written] == ['ulm/ulm_000001_000019_gtFine_labelIds.png', 'ulm/ulm_000002_000019_gtFine_labelIds.png',
                                                                  'bonn/bonn_000007_000019_gtFine_labelIds.png']
    assert sorted(os.listdir(os.path.join(result_dir, 'ulm'))) == ['ulm_%06d_000019_gtFine_labelIds.png' % s for s in (1, 2, 5)]
    got = hop_io.read_png(written[2])
    seg = model.predict_semantics({'ids': [7]}, None)['seg'][0].numpy()
    want = seg.astype(np.uint8) if no_convert else C.to_cityscapes(seg).astype(np.uint8)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    filled = hop_io.read_png(os.path.join(result_dir, 'ulm', 'ulm_000005_000019_gtFine_labelIds.png'))
    assert filled.shape == (1024, 2048) and (filled == (255 if no_convert else 0)).all()
    with pytest.raises(SystemExit, match='no_gpu'):
        export_semantic.export_split(model, StubDataset(), 'val', dict(params, no_gpu=True))


def test_export_semantic_takes_the_two_flags(tmp_path):
    from panoptic_forecasting_amd import config as pfconfig, export_semantic
    import yaml
    cfg = tmp_path / 'c.yaml'
    cfg.write_text(yaml.safe_dump({'task': 'fg', 'model': {}, 'data': {}, 'training': {'batch_size': 2}}))
    params = pfconfig.load_config(export_semantic.EXTRA_FLAGS, ['--config_file', str(cfg), '--export_name', 'sem', '--no_convert',
                                                                 '--working_dir', str(tmp_path)])
    assert params['export_name'] == 'sem' and params['no_convert'] is True
    params = pfconfig.load_config(export_semantic.EXTRA_FLAGS, ['--config_file', str(cfg), '--working_dir', str(tmp_path)])
    assert not params.get('export_name') and not params.get('no_convert')
