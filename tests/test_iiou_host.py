"""iIoU on the host: semantic_iou.instance_sums_host / iiou_from_sums / category_scores and the driver eval_semantic.py (host
matcher, instance files) against tests/iiou_ref64.py.  The per-image sums are float64 in a fixed order of operations and must be
EQUAL in bits, the counts equal; a derived score is a handful of fp64 operations on them: 1e-12 relative, the bar of
tests/test_semantic_iou_host.py for derived scores."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import conf_ref64 as C
import iiou_ref64 as R
import iiou_scenes as IS

REL = 1e-12
FMTS = ('trainid', 'cityscapes')
A_PERSON, A_RIDER, A_CAR, A_BUS = 3462.4756337644, 3930.4788056518, 12794.0202738185, 35732.1511111111
ORDER_SEED = 3                          # many_persons(ORDER_SEED): descending and ascending sums differ in bits (asserted below)
SHAPES = [((1, 1, 1), 1), ((2, 3, 5), 2), ((1, 7, 33), 3), ((3, 16, 64), 4), ((2, 127, 129), 5), ((2, 128, 128), 6), ((2, 5, 3277), 7),
          ((2, 200, 333), 8)]
OLD_KEYS = ['All', 'Stuff', 'MO', 'per_class', 'pixel_acc', 'confusion']


def host(pred, inst, n_cls=19, fmt='trainid'):
    from panoptic_forecasting_amd import semantic_iou as si
    sums, counts = si.instance_sums_host(torch.from_numpy(np.asarray(pred)), torch.from_numpy(np.asarray(inst)), n_cls, fmt)
    assert sums.dtype == torch.float64 and counts.dtype == torch.int64
    return sums.numpy(), counts.numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def hand_maps():
    """Two 4x8 images in Cityscapes format: the cases of the numbered list in the test below."""
    inst, pred = np.zeros((2, 4, 8), np.int64), np.zeros((2, 4, 8), np.int64)
    inst[0, 0, :] = 24001                       # 1. person of 8 pixels, 6 of them predicted person
    pred[0, 0, :6] = 24
    inst[0, 1, :5], pred[0, 1, :5] = 26002, 26  # 2. two cars: 5 of 5 ...
    inst[0, 1, 5:], pred[0, 1, 5:] = 26003, 24  #    ... and 0 of 3
    inst[0, 2, 0], pred[0, 2, 0] = 25007, 25    # 3. a rider of one pixel
    inst[0, 2, 1:3], pred[0, 2, 1:3] = 29001, 29     # 5. ignored: caravan, label 34, 1000, the largest u16, a car group
    inst[0, 2, 3:5], pred[0, 2, 3:5] = 34005, 34
    inst[0, 2, 5], inst[0, 2, 6], inst[0, 2, 7] = 1000, 65535, 26
    pred[0, 2, 5:] = 26
    inst[0, 3, :4], pred[0, 3, 0] = 28001, 28   # a bus of 4 pixels, 1 hit
    inst[0, 3, 4:] = 7
    inst[1, 0, :4], pred[1, 0, :4] = 24001, 24  # 4. the same id in another image: another instance
    return pred, inst


def test_hand_made_case_with_the_numbers_written_out():
    pred, inst = hand_maps()
    w_person, w_car5, w_car3, w_bus = A_PERSON / 8, A_CAR / 5, A_CAR / 3, A_BUS / 4
    want = np.zeros((2, 8, 2))
    want[0, 0] = 6 * w_person, 2 * w_person
    want[0, 1] = 1 * (A_RIDER / 1), 0.0
    want[0, 2] = (0.0 + 5 * w_car5) + 0 * w_car3, (0.0 + 0 * w_car5) + 3 * w_car3
    want[0, 4] = 1 * w_bus, 3 * w_bus
    want[1, 0] = 4 * (A_PERSON / 4), 0.0
    want_counts = np.zeros((2, 8, 3), np.int64)
    want_counts[0, 0], want_counts[0, 1], want_counts[0, 2], want_counts[0, 4], want_counts[1, 0] = (1, 8, 6), (1, 1, 1), (2, 8, 5), (1, 4, 1), (1, 4, 4)
    assert want[0, 0, 0] == 6 * (3462.4756337644 / 8) and want[0, 0, 1] == 2 * (3462.4756337644 / 8)
    for sums, counts in (R.instance_sums(pred, inst, 19, 'cityscapes'), host(pred, inst, 19, 'cityscapes')):
        assert same_bits(sums, want) and np.array_equal(counts, want_counts)
    sums, counts = host(pred, inst, 11, 'cityscapes')
    assert not sums.any() and not counts.any()
    sums, counts = host(pred, inst, 14, 'cityscapes')
    keep = np.zeros((2, 8, 2))
    keep[:, :3] = want[:, :3]
    assert same_bits(sums, keep) and not counts[:, 3:].any() and np.array_equal(counts[:, :3], want_counts[:, :3])
    assert same_bits(R.instance_sums(pred, inst, 14, 'cityscapes')[0], keep)
    # the same maps with a trainId prediction: person 11, car 13 (on the wrong car too), rider 12, bus 15
    train = np.full(pred.shape, 255, np.int64)
    for label, c in ((24, 11), (25, 12), (26, 13), (28, 15)):
        train[pred == label] = c
    sums, counts = host(train, inst, 19, 'trainid')
    assert same_bits(sums, want) and np.array_equal(counts, want_counts)


@pytest.mark.parametrize('fmt', FMTS)
def test_host_path_equals_the_restatement_bit_for_bit(fmt):
    pred, _, inst = IS.make_scenes(n=6)
    cases = [(pred, inst)] + [IS.inst_run_maps(shape, seed) for shape, seed in SHAPES]
    for p, i in cases:
        p = IS.in_format(p, fmt)
        want, want_counts = R.instance_sums(p, i, 19, fmt)
        sums, counts = host(p, i, 19, fmt)
        assert same_bits(sums, want) and np.array_equal(counts, want_counts), (fmt, p.shape)
    assert want_counts[:, :, 0].sum() > 8 and want_counts[:, :, 2].sum() > 0
    pred16, inst16 = IS.inst_run_maps((2, 16, 64), 4)
    from panoptic_forecasting_amd import semantic_iou as si
    assert (inst16 == 65535).any()
    for narrow in (inst16.astype(np.uint16).view(np.int16), inst16.astype(np.int32)):   # a 2-byte map is read as u16: 65535 stays
        got = si.instance_sums_host(torch.from_numpy(pred16), torch.from_numpy(narrow))
        assert same_bits(got[0].numpy(), R.instance_sums(pred16, inst16)[0]), narrow.dtype


def test_values_out_of_range_and_bad_arguments_raise():
    from panoptic_forecasting_amd import semantic_iou as si
    pred, inst = IS.inst_run_maps((1, 8, 8), 1)
    for bad_pred, bad_inst in ((256, None), (-1, None), (None, 65536), (None, -1), (None, 2 ** 33 + 5)):
        p, i = torch.from_numpy(pred).clone(), torch.from_numpy(inst).clone()
        if bad_pred is not None:
            p[0, 3, 3] = bad_pred
        else:
            i[0, 3, 3] = bad_inst
        with pytest.raises(ValueError, match='outside'):
            si.instance_sums_host(p, i)
    with pytest.raises(ValueError):
        si.instance_sums_host(torch.from_numpy(pred), torch.from_numpy(inst), fmt='coco')
    with pytest.raises(ValueError):
        si.instance_sums_host(torch.from_numpy(pred), torch.from_numpy(inst), n_cls=20)
    with pytest.raises(ValueError):
        si.instance_sums_host(torch.from_numpy(pred), torch.from_numpy(inst).float())
    with pytest.raises(ValueError):
        si.instance_sums_host(torch.from_numpy(pred), torch.from_numpy(inst)[:, :4])


def close(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= REL * abs(b)


def assert_scores(got_i, got_c, want_i, want_c):
    assert got_i['n'] == want_i['n'] and close(got_i['miou'], want_i['miou'])
    assert len(got_i['per_class']) == 8 and all(close(a, b) for a, b in zip(got_i['per_class'], want_i['per_class']))
    assert list(got_c['per_category']) == list(want_c['per_category']) == list(R.CATEGORY_CLASSES)
    for name, w in want_c['per_category'].items():
        assert close(got_c['per_category'][name]['iou'], w['iou']) and close(got_c['per_category'][name]['iiou'], w['iiou']), name
    for key in ('iou', 'iiou'):
        assert got_c[key]['n'] == want_c[key]['n'] and close(got_c[key]['miou'], want_c[key]['miou']), key


def test_scores_agree_with_the_restatement_and_keep_the_same_nan_books():
    from panoptic_forecasting_amd import semantic_iou as si
    pred, gt, inst = IS.make_scenes(n=6)
    table = C.confusion(pred, gt)[0]
    sums = R.running_sum(R.instance_sums(pred, inst)[0])
    assert (sums[:, 0] > 0).sum() >= 4
    for scale in (100.0, 1.0):
        assert_scores(si.iiou_from_sums(torch.from_numpy(table), torch.from_numpy(sums), scale),
                      si.category_scores(torch.from_numpy(table), torch.from_numpy(sums), scale),
                      R.iiou(table, sums, scale), R.categories(table, sums, scale))
    want = R.iiou(table, sums)
    assert 0 < want['n'] <= 8 and 0 < want['miou'] <= 100 and R.categories(table, sums)['iiou']['n'] == 2
    # a class without instances but with false positives scores 0; without either it is absent
    t = np.zeros((20, 20), np.int64)
    t[0, 0], t[0, 11], t[13, 13], t[2, 13], t[19, 14] = 50, 3, 10, 4, 6
    s = np.zeros((8, 2))
    s[2] = 7.5, 2.5
    got, ref = si.iiou_from_sums(torch.from_numpy(t), torch.from_numpy(s)), R.iiou(t, s)
    assert got['n'] == ref['n'] == 2 and got['per_class'][0] == 0.0 and got['per_class'][2] == 100.0 * (7.5 / 14.0)
    assert math.isnan(got['per_class'][3]) and math.isnan(ref['per_class'][3])
    assert_scores(got, si.category_scores(torch.from_numpy(t), torch.from_numpy(s)), ref, R.categories(t, s))
    cats = si.category_scores(torch.from_numpy(t), torch.from_numpy(s))
    assert cats['per_category']['flat']['iou'] == 100.0 * (50 / 53) and math.isnan(cats['per_category']['flat']['iiou'])
    assert cats['per_category']['vehicle']['iou'] == 100.0 * (10 / 14) and cats['per_category']['vehicle']['iiou'] == 100.0 * (7.5 / 14.0)
    assert cats['per_category']['human']['iou'] == 0.0 and cats['per_category']['human']['iiou'] == 0.0
    assert math.isnan(cats['per_category']['sky']['iou']) and cats['iou']['n'] == 4 and cats['iiou']['n'] == 2
    plain = si.category_scores(torch.from_numpy(t))
    assert plain['iiou']['n'] == 0 and math.isnan(plain['iiou']['miou']) and plain['iou'] == cats['iou']
    assert_scores(got, plain, ref, R.categories(t))
    empty = si.iiou_from_sums(torch.zeros(20, 20, dtype=torch.int64), torch.zeros(8, 2, dtype=torch.float64))
    assert empty['n'] == 0 and math.isnan(empty['miou'])


def test_the_sums_are_added_in_ascending_instance_value():
    pred, inst = IS.many_persons(ORDER_SEED)
    up, counts = R.instance_sums(pred, inst)
    down, _ = R.instance_sums(pred, inst, descending=True)
    assert counts[0, 0, 0] >= 200 and len(set(np.unique(inst, return_counts=True)[1].tolist())) > 50
    assert not same_bits(up[0, 0], down[0, 0])               # a condition on the input: the order shows in the bits
    assert same_bits(host(pred, inst)[0], up)


def test_the_table_and_the_status_bit_are_the_ones_the_header_documents():
    from panoptic_forecasting_amd import lib, semantic_iou as si
    text = open(os.path.join(ROOT, 'include', 'pfhip.h')).read()
    header = {name: int(v) for name, v in re.findall(r'^#define (PF_IIOU_STATUS_[A-Z]+) (\d+)u$', text, re.M)}
    assert header == {'PF_IIOU_STATUS_VALUE': 1}
    assert {t.split(':')[0]: bit for bit, t in si.IIOU_STATUS_BITS} == header
    assert lib.load().pf_iiou_chunk_pixels() == 16384 and re.search(r'pf_iiou_chunk_pixels\(\) = 16384', text)
    assert list(si.AVG_CLASS_SIZE) == [R.AVG[c] for c in range(11, 19)]
    kernel = open(os.path.join(ROOT, 'panoptic-forecasting_amd', 'csrc', 'iiou_kernels.hip')).read()
    block = kernel[kernel.index('kIiouAvgSize[kIiouThings] = {'):]
    assert [float(x) for x in re.findall(r'[0-9]+\.[0-9]+', block[:block.index('}')])] == list(si.AVG_CLASS_SIZE)
    assert [(n, list(m)) for n, m in si.CATEGORIES] == [(n, m) for n, m in R.CATEGORY_CLASSES.items()]


def run_driver(flags, out, *extra):
    from panoptic_forecasting_amd import eval_semantic
    res = eval_semantic.run(eval_semantic.parse_args(flags + ['--results_file', out, '--matcher', 'host', '--batch_size', '2',
                                                              '--num_workers', '2'] + list(extra)))
    with open(out) as f:
        doc = json.load(f)
    assert doc == json.loads(json.dumps(res))
    return doc


def test_driver_without_instance_files_writes_the_file_it_wrote_before(tmp_path, capsys):
    from panoptic_forecasting_amd import eval_semantic
    pred, gt, inst = IS.make_scenes(n=3, h=32, w=48, seed=9)
    flags = IS.write_tree(str(tmp_path), pred, gt, inst, 'cityscapes', only=())
    auto = run_driver(flags, str(tmp_path / 'auto.json'))
    table_auto = capsys.readouterr().out
    off = run_driver(flags, str(tmp_path / 'off.json'), '--instances', 'off')
    assert auto == off and list(auto) == OLD_KEYS and table_auto == capsys.readouterr().out and 'iIoU' not in table_auto
    assert open(str(tmp_path / 'auto.json')).read() == open(str(tmp_path / 'off.json')).read()
    assert np.array_equal(np.array(auto['confusion']), C.confusion(pred, gt)[0])
    with pytest.raises(eval_semantic.EvalError, match='no instance map .*city0_000000_000019_gtFine_instanceIds.png'):
        run_driver(flags, str(tmp_path / 'r.json'), '--instances', 'require')


@pytest.mark.parametrize('fmt', FMTS)
def test_driver_with_instance_files_carries_the_restatements_numbers(tmp_path, fmt, capsys):
    pred, gt, inst = IS.make_scenes(n=3, h=32, w=48, seed=9)
    flags = IS.write_tree(str(tmp_path), pred, gt, inst, fmt)
    assert os.path.isfile(os.path.join(str(tmp_path), 'gt', 'city0', 'city0_000000_000019_gtFine_' +
                                       ('labelIds.png' if fmt == 'cityscapes' else 'labelTrainIds.png')))
    doc = run_driver(flags, str(tmp_path / 'res.json'))
    off = run_driver(flags, str(tmp_path / 'off.json'), '--instances', 'off')
    assert list(doc) == OLD_KEYS + ['iIoU', 'instances', 'categories'] and {k: doc[k] for k in OLD_KEYS} == off
    per, counts = R.instance_sums(IS.in_format(pred, fmt), inst, 19, fmt)
    table, sums = C.confusion(pred, gt)[0], R.running_sum(per)
    want_i, want_c = R.iiou(table, sums, 1.0), R.categories(table, sums, 1.0)
    nan = lambda x: float('nan') if x is None else x
    names = list(doc['per_class'])[11:]
    assert list(doc['iIoU']['per_class']) == names == list(doc['instances']) and want_i['n'] > 0
    got_i = {'miou': nan(doc['iIoU']['miou']), 'n': doc['iIoU']['n'], 'per_class': [nan(x) for x in doc['iIoU']['per_class'].values()]}
    cats = {k: v for k, v in doc['categories'].items() if k not in ('iou', 'iiou')}
    got_c = {'per_category': {k: {'iou': nan(v['iou']), 'iiou': nan(v['iiou'])} for k, v in cats.items()},
             'iou': {'miou': nan(doc['categories']['iou']), 'n': want_c['iou']['n']},
             'iiou': {'miou': nan(doc['categories']['iiou']), 'n': want_c['iiou']['n']}}
    assert_scores(got_i, got_c, want_i, want_c)
    assert [doc['instances'][n] for n in names] == [{'n': int(r[0]), 'pixels': int(r[1])} for r in counts.sum(0)]
    assert all(cats[k]['iiou'] is None for k in ('flat', 'construction', 'object', 'nature', 'sky'))
    printed = capsys.readouterr().out
    assert 'iIoU' in printed and 'vehicle' in printed and 'categories' in printed


def test_driver_refuses_a_mixed_tree_and_bad_instance_files(tmp_path):
    from PIL import Image
    from panoptic_forecasting_amd import eval_semantic
    pred, gt, inst = IS.make_scenes(n=3, h=32, w=48, seed=9)
    root = str(tmp_path)
    flags = IS.write_tree(root, pred, gt, inst, 'cityscapes', only=(0, 2))
    out = str(tmp_path / 'r.json')
    for mode in ('auto', 'require'):
        with pytest.raises(eval_semantic.EvalError, match='no instance map .*city1_000001_000019_gtFine_instanceIds.png'):
            run_driver(flags, out, '--instances', mode)
    assert list(run_driver(flags, out, '--instances', 'off')) == OLD_KEYS
    victim = IS.instance_file(root, 1)
    Image.fromarray(np.zeros((32, 47), np.uint16)).save(victim)
    with pytest.raises(eval_semantic.EvalError, match='city1_000001.*ground truth is 32x48, instance map .*city1_000001_000019_gtFine_instanceIds.png 32x47'):
        run_driver(flags, out)
    Image.fromarray(np.zeros((32, 48, 3), np.uint8)).save(victim)
    with pytest.raises(eval_semantic.EvalError, match='city1_000001_000019_gtFine_instanceIds.png is not a single-channel 16-bit or 32-bit'):
        run_driver(flags, out)
    Image.fromarray(np.zeros((32, 48), np.uint8)).save(victim)
    with pytest.raises(eval_semantic.EvalError, match='city1_000001_000019_gtFine_instanceIds.png is not a single-channel 16-bit or 32-bit'):
        run_driver(flags, out)
    Image.fromarray(inst[1].astype(np.uint16)).save(victim)
    whole = run_driver(flags, out)
    flags16 = IS.write_tree(str(tmp_path / 'all16'), pred, gt, inst, 'cityscapes')
    assert whole == run_driver(flags16, str(tmp_path / 'r16.json')) and whole['iIoU']['n'] > 0


def test_two_gloo_ranks_give_the_single_process_file(tmp_path):
    import iiou_eval_worker
    pred, gt, inst = IS.make_scenes(n=5, h=32, w=48, seed=9)
    flags = IS.write_tree(str(tmp_path), pred, gt, inst, 'cityscapes')
    one, two = str(tmp_path / 'one.json'), str(tmp_path / 'two.json')
    a = run_driver(flags, one)
    iiou_eval_worker.spawn_two(flags + ['--results_file', two, '--matcher', 'host', '--batch_size', '2', '--num_workers', '2'])
    with open(two) as f:
        b = json.load(f)
    assert a == b and a['iIoU']['n'] > 0 and open(one).read() == open(two).read()
