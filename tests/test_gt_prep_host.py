"""Ground-truth preparation on the host: gt_prep.prepare_host / remove_fg_host / segments_info and the driver prepare_gt.py
(--backend host) against the per-segment restatement tests/gtprep_ref.py, the reference's own remove_fg_from_gt.py (fixture G14) and
the evaluators and the dataset that read what the driver writes.  Everything is integers: every comparison is equality."""
import ctypes
import json
import os
import re
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import gtprep_ref as R
import gtprep_scenes as S
from panoptic_forecasting_amd import eval_common, gt_prep, hop_io, lib, panoptic


def scenes():
    maps = dict(S.hand_made())
    maps.update(odd=S.blocky(37, 53, 1), worst=S.worst_case_96x256(), street=S.blocky(64, 128, 2, n_things=60))
    return maps


def assert_matches_ref(res, b, ref):
    assert np.array_equal(np.asarray(res['panoptic'][b]), ref['rgb'])
    assert np.array_equal(np.asarray(res['trainids'][b]), ref['train'])
    assert np.array_equal(np.asarray(res['nofg'][b]), ref['nofg'])
    rows = gt_prep.segment_rows(res)[b]
    assert rows.tolist() == ref['rows']
    assert gt_prep.segments_info(rows) == ref['info']


@pytest.mark.parametrize('name', sorted(scenes()))
def test_prepare_host_equals_the_per_segment_restatement(name):
    m = scenes()[name]
    ref = R.prepare_image(m)
    assert not ref['flagged'] and ref['rows']
    for dtype in (np.uint16, np.int16, np.int32, np.int64):
        assert_matches_ref(gt_prep.prepare_host(m.astype(np.uint16).view(np.int16) if dtype == np.int16 else m.astype(dtype)), 0, ref)


def test_the_hand_made_maps_say_what_they_are_for():
    hm = {k: R.prepare_image(v) for k, v in S.hand_made().items()}
    assert {'id': 26, 'category_id': 26, 'area': 6, 'bbox': [2, 1, 3, 2], 'iscrowd': 1} in hm['crowd']['info']
    assert {'id': 7001, 'category_id': 7, 'area': 6, 'bbox': [0, 0, 8, 4], 'iscrowd': 0} in hm['stuff_instance']['info']
    assert [r[0] for r in hm['ignored']['rows']] == [7]
    assert (hm['ignored']['train'][:2, :2] == 255).all() and not hm['ignored']['rgb'][:2, :2].any() and not hm['ignored']['rgb'][3].any()
    assert [r[0] for r in hm['index_999']['rows']] == [7, 24000, 24999, 33999]
    assert [25001, 1, 5, 2, 1, 1] in hm['one_pixel']['rows'] and [23, 1, 7, 0, 1, 1] in hm['one_pixel']['rows']
    assert [26005, 20, 0, 0, 8, 4] in hm['borders']['rows']
    # the colour of an id is its three low bytes
    assert hm['index_999']['rgb'][2, 2].tolist() == [33999 % 256, 33999 // 256 % 256, 0]


def test_segments_info_with_train_ids_and_batches():
    maps = np.stack([S.blocky(16, 24, s, n_things=6, block=4) for s in (3, 4, 5)])
    res = gt_prep.prepare_host(maps)
    for b in range(3):
        assert_matches_ref(res, b, R.prepare_image(maps[b]))
    rows = gt_prep.segment_rows(res)[0]
    for a, t in zip(gt_prep.segments_info(rows), gt_prep.segments_info(rows, use_train_id=True)):
        assert t['category_id'] == R.LABEL_FACTS[a['category_id']][0] and {k: v for k, v in a.items() if k != 'category_id'} == \
            {k: v for k, v in t.items() if k != 'category_id'}
    only = gt_prep.prepare_host(maps, want=('nofg',))
    assert sorted(only) == ['nofg'] and np.array_equal(only['nofg'], res['nofg'])


def test_remove_fg_host_equals_the_reference_script():
    g = np.load(os.path.join(GOLDEN, 'g14_gtprep.npz'))
    assert len(np.unique(g['inputs'])) == 256 and (g['inputs'] != g['outputs']).any()
    assert np.array_equal(gt_prep.remove_fg_host(g['inputs']), g['outputs'])
    assert gt_prep.MOVING_TRAIN_IDS == tuple(range(11, 19))
    with pytest.raises(lib.PfError, match='8-bit'):
        gt_prep.remove_fg_host(g['inputs'].astype(np.int32))


def test_label_tables_agree():
    """csrc/gt_labels.h (through pf_debug_gt_labels) == gt_prep.LABELS == what panoptic.TRAINID2ID, eval_common.LABEL_NAMES and
    the restatement's own facts say."""
    L = lib.load()
    out8, name, cat = (ctypes.c_int * 8)(), ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    device = []
    for i in range(len(gt_prep.LABELS)):
        assert L.pf_debug_gt_labels(i, out8, name, 64, cat, 64) == 0
        v = list(out8)
        device.append(gt_prep.Label(name.value.decode(), v[0], v[1], cat.value.decode(), v[2], bool(v[3]), bool(v[4]), tuple(v[5:8])))
    assert L.pf_debug_gt_labels(len(gt_prep.LABELS), out8, name, 64, cat, 64) != 0 and L.pf_debug_gt_labels(-1, out8, name, 64, cat, 64) != 0
    assert tuple(device) == gt_prep.LABELS and len(device) == 35
    with_train = sorted((l.train_id, l.id, l.name) for l in gt_prep.LABELS if 0 <= l.train_id < 255)
    assert tuple(i for _, i, _ in with_train) == panoptic.TRAINID2ID
    assert tuple(n for _, _, n in with_train) == eval_common.LABEL_NAMES
    assert [l.id for l in gt_prep.LABELS[:34]] == list(range(34)) and gt_prep.LABELS[34].id == -1
    assert {l.id: (l.train_id, int(l.has_instances), int(l.ignore_in_eval)) for l in gt_prep.LABELS[:34]} == R.LABEL_FACTS
    cats = gt_prep.categories()
    assert [c['id'] for c in cats] == list(panoptic.TRAINID2ID) and [c['isthing'] for c in cats] == [0] * 11 + [1] * 8
    assert [c['id'] for c in gt_prep.categories(use_train_id=True)] == list(range(19))


def test_header_and_python_name_the_same_status_bits():
    text = open(os.path.join(ROOT, 'include', 'pfhip.h')).read()
    header = {name: int(v) for name, v in re.findall(r'^#define (PF_GTPREP_STATUS_[A-Z]+) (\d+)u$', text, re.M)}
    assert header == {'PF_GTPREP_STATUS_FULL': 1, 'PF_GTPREP_STATUS_VALUE': 2}
    assert {t.split(':')[0]: bit for bit, t in gt_prep.STATUS_BITS} == header
    assert gt_prep.max_segments() == 1024 and re.search(r'pf_gt_prepare_max_segments\(\) = 1024', text)
    need = ctypes.c_size_t()
    assert lib.load().pf_gt_prepare_workspace(2, ctypes.byref(need)) == 0 and need.value >= 256 + 2 * 5 * 33034 * 4
    assert lib.load().pf_gt_prepare_workspace(-1, ctypes.byref(need)) == -1


@pytest.mark.parametrize('bad', [(40, np.int64), (34000, np.int64), (34000, np.uint16), (-7, np.int32), (999, np.int32),
                                 (2 ** 33 + 7, np.int64), (65535, np.uint16)])
def test_illegal_values_are_refused_by_name(bad):
    value, dtype = bad
    m = np.full((2, 4, 8), 7, dtype)
    m[1, 2, 3] = value
    with pytest.raises(lib.PfError, match=r'PF_GTPREP_STATUS_VALUE.*image 1 of the batch'):
        gt_prep.prepare_host(m)
    with pytest.raises(lib.PfError, match=r'PF_GTPREP_STATUS_VALUE'):
        gt_prep.prepare_host(m, want=('trainids',))


def test_more_segments_than_the_list_holds_is_refused_by_name():
    cap = gt_prep.max_segments()
    assert len(gt_prep.segment_rows(gt_prep.prepare_host(S.many_ids(64, 64, cap)))[0]) == cap
    with pytest.raises(lib.PfError, match='PF_GTPREP_STATUS_FULL'):
        gt_prep.prepare_host(S.many_ids(64, 64, cap + 1))
    assert gt_prep.prepare_host(S.many_ids(64, 64, cap + 1), want=('trainids', 'nofg'))['trainids'].shape == (1, 64, 64)


def test_a_cpu_device_is_refused():
    with pytest.raises(lib.PfError, match='prepare_host'):
        gt_prep.GTPreparer('cpu')


# ---------------------------------------------------------------------------------------------- the driver
def tree_maps():
    return [S.blocky(24, 40, s, n_things=10, block=8) for s in (11, 12, 13)] + [S.hand_made()['crowd'].repeat(6, 0).repeat(5, 1)]


def all_files(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), 'rb').read() for d, _, fs in os.walk(root) for f in fs}


def test_driver_round_trip_on_a_tiny_tree(tmp_path, capsys):
    from panoptic_forecasting_amd import bg_dataset, eval_panoptic, eval_semantic, prepare_gt
    maps = tree_maps()
    gtfine, nofg, out = str(tmp_path / 'gtFine'), str(tmp_path / 'nofg'), str(tmp_path / 'pan')
    files = S.write_tree(gtfine, maps, 'val')
    S.write_tree(gtfine, maps[:1], 'train', bits=32)
    common = ['--backend', 'host', '--batch_size', '3', '--num_workers', '2']
    prepare_gt.main(['all', '--dataset-folder', gtfine, '--nofg-output', nofg, '--output-folder', out] + common)
    printed = capsys.readouterr().out
    assert 'set test: no <city>/*_gtFine_instanceIds.png' in printed and 'skipped' in printed and 'set val: 4 images' in printed
    # the JSON: fields, their order, images in sorted file order
    with open(os.path.join(out, 'cityscapes_panoptic_val.json')) as f:
        doc = json.load(f)
    assert list(doc) == ['images', 'annotations', 'categories']
    bases = [os.path.basename(f)[:-len('_gtFine_instanceIds.png')] for f in files]
    by_base = {os.path.basename(f)[:-len('_gtFine_instanceIds.png')]: m for f, m in
               zip(sorted(files, key=lambda f: int(os.path.basename(f).split('_')[1])), maps)}
    assert [im['id'] for im in doc['images']] == bases == sorted(bases)
    assert doc['images'][0] == {'id': bases[0], 'width': 40, 'height': 24, 'file_name': bases[0] + '_gtFine_leftImg8bit.png'}
    assert list(doc['images'][0]) == ['id', 'width', 'height', 'file_name']
    assert doc['categories'] == gt_prep.categories() and list(doc['categories'][0]) == ['id', 'name', 'color', 'supercategory', 'isthing']
    assert sorted(os.listdir(os.path.join(out, 'cityscapes_panoptic_val'))) == [b + '_gtFine_panoptic.png' for b in bases]
    for ann, base in zip(doc['annotations'], bases):
        ref = R.prepare_image(by_base[base])
        assert list(ann) == ['image_id', 'file_name', 'segments_info'] and ann['image_id'] == base
        assert ann['file_name'] == base + '_gtFine_panoptic.png' and ann['segments_info'] == ref['info']
        assert list(ann['segments_info'][0]) == ['id', 'category_id', 'area', 'bbox', 'iscrowd']
        png = hop_io.read_png(os.path.join(out, 'cityscapes_panoptic_val', ann['file_name']))
        assert np.array_equal(png, ref['rgb'])
        ids = panoptic.decode_png(png)
        listed = np.isin(by_base[base], [r[0] for r in ref['rows']])
        assert np.array_equal(ids[listed], by_base[base][listed]) and not ids[~listed].any()
        city = base.split('_')[0]
        assert np.array_equal(hop_io.read_png(os.path.join(gtfine, 'val', city, base + '_gtFine_labelTrainIds.png')), ref['train'])
        assert np.array_equal(hop_io.read_png(os.path.join(nofg, 'val', city, base + '_gtFine_labelTrainIds.png')), ref['nofg'])
    assert os.path.isfile(os.path.join(out, 'cityscapes_panoptic_train.json'))           # the 32-bit instance PNG of the train set
    # the panoptic evaluator accepts the ground truth; a prediction that is a copy of it scores 1 in every class present
    gt_json = os.path.join(out, 'cityscapes_panoptic_val.json')
    res = eval_panoptic.run(eval_panoptic.parse_args(['--gt-json-file', gt_json, '--prediction-json-file', gt_json, '--matcher', 'host',
                                                      '--results_file', str(tmp_path / 'pq.json'), '--num_workers', '2']))
    present = {R.LABEL_FACTS[R.label_of(s['id'])][0] for a in doc['annotations'] for s in a['segments_info'] if not s['iscrowd']}
    assert res['All']['n'] == len(present) > 8
    for t, name in enumerate(eval_common.LABEL_NAMES):
        want = 1.0 if t in present else 0.0
        assert res['per_class'][name] == {'pq': want, 'sq': want, 'rq': want}, name
    assert res['All']['pq'] == res['All']['sq'] == res['All']['rq'] == 1.0
    # the semantic evaluator accepts the trainId tree: against itself every class present has IoU 1
    sem = eval_semantic.run(eval_semantic.parse_args(['--gt-folder', os.path.join(gtfine, 'val'), '--prediction-folder',
                                                      os.path.join(gtfine, 'val'), '--format', 'trainid', '--matcher', 'host',
                                                      '--results_file', str(tmp_path / 'iou.json'), '--num_workers', '2']))
    assert sem['All']['miou'] == 1.0 and sem['All']['n'] > 8
    # bg training's dataset enumerates the no-foreground tree
    data = str(tmp_path / 'data')
    for base in bases:
        city = base.split('_')[0]
        os.makedirs(os.path.join(data, 'val', city), exist_ok=True)
        hop_io.write_png(os.path.join(data, 'val', city, base + '_gtFine_labelIds.png'), np.zeros((24, 40), np.uint8))
    ds = bg_dataset.NativeBGDataset('val', {'data': {'data_dir': [data] * 3, 'gt_dir': nofg, 'use_depths': False, 'only_background': True,
                                                     'gap_len': [3]}})
    assert [os.path.basename(s['gt_file']) for s in ds.samples] == [b + '_gtFine_labelTrainIds.png' for b in bases]
    assert ds.source_shape() == (24, 40)
    # the `all` route and the `trainids` + `remove_fg` route write identical bytes; so does a rerun over existing outputs
    gt2, nofg2 = str(tmp_path / 'gtFine2'), str(tmp_path / 'nofg2')
    S.write_tree(gt2, maps, 'val')
    prepare_gt.main(['trainids', '--dataset-folder', gt2, '--set-names', 'val'] + common)
    prepare_gt.main(['remove_fg', '--input_dir', os.path.join(gt2, 'val'), '--output_dir', os.path.join(nofg2, 'val')] + common)
    assert all_files(os.path.join(gt2, 'val')) == all_files(os.path.join(gtfine, 'val'))
    assert all_files(nofg2) == {k: v for k, v in all_files(nofg).items() if k.startswith('val')} and len(all_files(nofg2)) == 4
    before = all_files(out)
    prepare_gt.main(['panoptic', '--dataset-folder', gtfine, '--output-folder', out, '--set-names', 'val', '--use-train-id'] + common)
    prepare_gt.main(['panoptic', '--dataset-folder', gtfine, '--output-folder', out, '--set-names', 'val'] + common)
    after = all_files(out)
    assert {k: v for k, v in after.items() if '_trainId' not in k} == before
    with open(os.path.join(out, 'cityscapes_panoptic_val_trainId.json')) as f:
        tdoc = json.load(f)
    assert tdoc['categories'] == gt_prep.categories(use_train_id=True)
    assert [s['category_id'] for s in tdoc['annotations'][0]['segments_info']] == \
        [R.LABEL_FACTS[s['category_id']][0] for s in doc['annotations'][0]['segments_info']]
    assert after[os.path.join('cityscapes_panoptic_val_trainId', bases[0] + '_gtFine_panoptic.png')] == \
        after[os.path.join('cityscapes_panoptic_val', bases[0] + '_gtFine_panoptic.png')]


def test_driver_refuses_bad_files_by_name(tmp_path):
    from PIL import Image
    from panoptic_forecasting_amd import prepare_gt
    gtfine = str(tmp_path / 'gtFine')
    m = np.full((4, 8), 7, np.int64)
    files = S.write_tree(gtfine, [m, m], 'val')
    bad = m.copy()
    bad[1, 1] = 40
    Image.fromarray(bad.astype(np.uint16)).save(files[1])
    with pytest.raises(SystemExit, match=r'prepare_gt: set val.*PF_GTPREP_STATUS_VALUE'):
        prepare_gt.main(['trainids', '--dataset-folder', gtfine, '--set-names', 'val', '--backend', 'host'])
    Image.fromarray(np.zeros((4, 8), np.uint8)).save(files[1])
    with pytest.raises(SystemExit, match='not a single-channel 16-bit or 32-bit instance PNG'):
        prepare_gt.main(['trainids', '--dataset-folder', gtfine, '--set-names', 'val', '--backend', 'host'])
    shutil.rmtree(gtfine)
    with pytest.raises(SystemExit, match='no input folder'):
        prepare_gt.main(['remove_fg', '--input_dir', os.path.join(gtfine, 'val'), '--output_dir', str(tmp_path / 'o')])
