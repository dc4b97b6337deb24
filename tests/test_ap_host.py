"""Instance AP on the host: instance_ap.records_host + ap_from_records against tests/ap_ref64.py (the original's pairwise
matching in plain loops).  Lists are compared as multisets, hard_fn as integers, AP as bits."""
import math
import struct

import numpy as np
import pytest

import ap_ref64 as R
import ap_scenes as S


def bits(x):
    return struct.pack('<d', float(x))


def same_ap(a, b):
    return all(bits(x) == bits(y) for ra, rb in zip(a, b) for x, y in zip(ra, rb)) and len(a) == len(b)


WORKED = [([(1, 1.0)], 0, 1.0), ([(1, .9), (0, .8)], 0, 1.0), ([(1, .9), (0, .95)], 0, 0.25), ([(1, .9), (0, .9)], 0, 0.75),
          ([(1, .5)], 1, 0.5), ([(1, .9), (1, .7), (0, .8)], 1, 0.5277777777777777)]


@pytest.mark.parametrize('pairs,hard_fn,want', WORKED)
def test_worked_values_bit_for_bit(pairs, hard_fn, want):
    from panoptic_forecasting_amd import instance_ap as ia
    got = ia.average_precision([t for t, _ in pairs], [s for _, s in pairs], hard_fn)
    assert bits(got) == bits(want), (got, want)
    assert bits(ia.average_precision([t for t, _ in pairs[::-1]], [s for _, s in pairs[::-1]], hard_fn)) == bits(want)
    assert bits(R.curve([t for t, _ in pairs], [s for _, s in pairs], hard_fn)) == bits(want)


def test_thresholds_are_the_arange_values():
    from panoptic_forecasting_amd import instance_ap as ia
    assert ia.THRESHOLDS == tuple(np.arange(0.5, 1.0, 0.05).tolist()) and len(ia.THRESHOLDS) == 10
    assert ia.THRESHOLDS[2] == 0.6000000000000001 and ia.THRESHOLDS[0] == 0.5
    assert not 3 / 5 > ia.THRESHOLDS[2] and 60.0 / 100 == 3 / 5


def test_the_label_tables_agree_with_the_projects_label_table():
    from panoptic_forecasting_amd import gt_prep, instance_ap as ia, panoptic
    assert ia.INSTANCE_LABELS == tuple(panoptic.TRAINID2ID[11:19]) == R.INSTANCE_LABELS
    void = tuple(sorted(l[1] for l in gt_prep.LABELS if l[1] >= 0 and l[6]))
    assert void == ia.VOID_IDS == R.VOID_IDS
    from panoptic_forecasting_amd import eval_common
    assert ia.CLASS_NAMES == eval_common.LABEL_NAMES[11:] == R.CLASS_NAMES


def compare(scene, min_region):
    from panoptic_forecasting_amd import instance_ap as ia
    masks, image, labels, scores, gt = scene
    rec, regular = ia.records_host(masks, image, labels, gt, min_region)
    got = ia.ap_from_records(rec, regular, scores, None, min_region)
    lists, _, _ = ia.match_lists(rec, regular, scores, None, min_region)
    want = R.evaluate(S.per_image(masks, image, labels, scores, gt), min_region)
    for key, (pairs, hard_fn) in want['lists'].items():
        y_true, y_score, fn = lists[key]
        assert sorted(zip(y_true, y_score)) == pairs, (key, min_region)
        assert fn == hard_fn, (key, min_region)
    assert same_ap(got['ap'], want['ap']), min_region
    assert bits(got['allAp']) == bits(want['allAp']) and bits(got['allAp50%']) == bits(want['allAp50%'])
    for name in R.CLASS_NAMES:
        assert bits(got['classes'][name]['ap']) == bits(want['classes'][name]['ap'])
        assert bits(got['classes'][name]['ap50%']) == bits(want['classes'][name]['ap50%'])
    return rec.numpy(), regular.numpy(), got, lists


@pytest.mark.parametrize('min_region', [1, 3, 100])
def test_hand_scene_equals_the_restatement(min_region):
    from panoptic_forecasting_amd import instance_ap as ia
    masks, image, labels, scores, gt, notes = S.hand_scene()
    rec, regular, got, lists = compare((masks, image, labels, scores, gt), min_region)
    r = lambda name: rec[notes[name]].tolist()
    # the records say what the scene was built to say
    assert r('exact') == [0, 300, 0, 26001, 300, 300, 0, 2] and r('duplicate') == [0, 200, 0, 26001, 200, 300, 0, 2]
    assert r('hits group') == [0, 180, 180, 24, 180, 200, 0, 0]
    assert r('hits small') == [0, 50, 50 if min_region == 100 else 0, 25001, 50, 50, 0, 1]
    assert r('void just below')[:3] == [0, 201, 100] and r('void just above')[:3] == [0, 199, 100]
    assert r('small group') == [0, 25, 20 if min_region == 100 else 10, 33, 10, 10, 0, 7]
    assert r('exactly 0.5')[3:6] == [32001, 50, 100] and r('exactly 0.75')[3:6] == [32002, 75, 100] and r('exactly 3/5')[3:6] == [28001, 60, 100]
    assert r('empty') == [1, 0, 0, -1, 0, 0, 0, 2]
    assert r('stuff label') == [2, 0, 0, -1, 0, 0, 0, -1] and r('caravan label') == [2, 0, 0, -1, 0, 0, 0, -1]
    assert r('tiny') == [0, 2, 2 if min_region > 2 else 0, 27001, 2, 2, 0, 3]
    assert r('mixed') == [0, 170, 50, 26001, 50, 300, 0, 2]
    assert r('no ground truth') == [0, 190, 0, -1, 0, 0, 2, 2]
    assert regular[1].tolist() == [0, 0, 1, 0, 0, 1, 0, 0] and regular[2].tolist() == [0] * 8
    assert regular[0].tolist() == [0, 0 if min_region == 100 else 1, 1, 1 if min_region < 3 else 0, 1, 0, 2, 0]
    # and the lists what the definition says: car at t = 0.5 and 0.7, motorcycle at 0.5, bus at 0.6000000000000001
    car50 = sorted(zip(*lists[(2, 0)][:2]))
    assert car50 == sorted([(1, 0.9), (0, 0.8), (0, 0.5), (0, 0.35), (0, 0.3)]) and lists[(2, 0)][2] == 1        # 'void just above' dropped
    assert (0, 0.45) in sorted(zip(*lists[(2, 1)][:2]))                                                          # ... and back at 0.55
    assert sorted(zip(*lists[(2, 4)][:2])) == sorted([(1, 0.9), (0, 0.8), (0, 0.5), (0, 0.45), (0, 0.35), (0, 0.3)])
    assert sorted(zip(*lists[(6, 0)][:2])) == [(0, 0.95), (1, 0.85)] and lists[(6, 0)][2] == 1                  # 0.5 is no hit
    assert sorted(zip(*lists[(4, 1)][:2])) == [(1, 0.75)] and sorted(zip(*lists[(4, 2)][:2])) == [(0, 0.75)]    # 3/5 at 0.6000000000000001
    assert lists[(0, 0)][:2] == ([], []) and lists[(0, 9)][:2] == ([], [])                                      # the group's hit and its ignore share
    assert [x for x in lists[(7, 5)][1]] == ([] if min_region == 100 else [0.4]) and lists[(7, 6)][1] == [0.4]  # 20 / 25 <= 0.8
    assert math.isnan(got['classes']['person']['ap']) and math.isnan(got['classes']['bicycle']['ap'])           # groups only: no gt
    assert got['classes']['train']['ap'] == 0.0                                                                 # gt and no prediction
    assert math.isnan(got['classes']['rider']['ap']) == (min_region == 100)
    assert got['classes']['truck']['ap'] == 1.0 if min_region == 1 else math.isnan(got['classes']['truck']['ap'])
    assert 0.0 < got['allAp'] < 1.0


@pytest.mark.parametrize('min_region', [1, 3, 100])
def test_random_scenes_equal_the_restatement(min_region):
    for seed, shape, p in ((1, (3, 16, 64), 12), (2, (2, 40, 50), 10), (3, (1, 3, 5), 4)):
        gt, masks, image, labels, scores = S.random_scene(shape, seed, p)
        compare((masks, image, labels, scores, gt), min_region)


def test_every_prediction_dropped_is_zero_where_the_original_would_raise():
    from panoptic_forecasting_amd import instance_ap as ia
    gt = np.full((1, 20, 20), 7, np.int64)
    gt[0, :10] = 26001                                   # 200 pixels, regular
    gt[0, 10:] = 0                                       # void
    mask = np.zeros((1, 20, 20), np.uint8)
    mask[0, 10:] = 1                                     # all over void: dropped at every threshold
    rec, regular = ia.records_host(mask, [0], [26], gt)
    res = ia.ap_from_records(rec, regular, [0.9])
    assert res['classes']['car'] == {'ap': 0.0, 'ap50%': 0.0}
    assert R.evaluate(S.per_image(mask, [0], [26], [0.9], gt))['classes']['car']['ap'] == 0.0


def test_order_invariance_same_bits():
    from panoptic_forecasting_amd import instance_ap as ia
    gt, masks, image, labels, scores = S.random_scene((3, 16, 64), 5, 40)
    rec, regular = ia.records_host(masks, image, labels, gt, 3)
    base = ia.ap_from_records(rec, regular, scores, None, 3)
    assert 0 < base['allAp'] < 1
    rng = np.random.default_rng(0)
    for _ in range(3):
        perm = rng.permutation(len(rec))
        again = ia.ap_from_records(rec[perm], regular[[2, 0, 1]], scores[perm], None, 3)
        assert same_ap(again['ap'], base['ap']) and bits(again['allAp']) == bits(base['allAp'])


def test_image_offsets_tell_the_images_of_two_calls_apart():
    from panoptic_forecasting_amd import instance_ap as ia
    masks, image, labels, scores, gt, _ = S.hand_scene()
    rec, regular = ia.records_host(masks, image, labels, gt, 3)
    whole = ia.ap_from_records(rec, regular, scores, None, 3)
    recs, regs, offs = [], [], []
    for i in range(3):                                   # one call per image: every record says image 0
        sel = np.nonzero(image == i)[0]
        r, g = ia.records_host(masks[sel], np.zeros(len(sel), np.int32), labels[sel], gt[i:i + 1], 3)
        assert np.array_equal(r[:, :6].numpy(), rec[sel][:, :6].numpy()) and np.array_equal(g[0].numpy(), regular[i].numpy())
        recs.append(r.numpy())
        regs.append(g.numpy())
        offs += [i] * len(sel)
    order = np.concatenate([np.nonzero(image == i)[0] for i in range(3)])
    split = ia.ap_from_records(np.concatenate(recs), np.concatenate(regs), scores[order], offs, 3)
    assert same_ap(split['ap'], whole['ap'])


def test_host_refusals_and_the_id_map_expansion():
    import torch
    from panoptic_forecasting_amd import instance_ap as ia, lib
    gt = np.full((1, 4, 4), 7, np.int64)
    m = np.ones((1, 4, 4), np.uint8)
    with pytest.raises(lib.PfError, match='PF_AP_STATUS_VALUE'):
        ia.records_host(m, [0], [26], np.full((1, 4, 4), 65536, np.int64))
    with pytest.raises(lib.PfError, match='PF_AP_STATUS_VALUE'):
        ia.records_host(m, [0], [26], np.full((1, 4, 4), -1, np.int64))
    with pytest.raises(lib.PfError, match='PF_AP_STATUS_INDEX'):
        ia.records_host(m, [1], [26], gt)
    with pytest.raises(lib.PfError, match='PF_AP_STATUS_INDEX'):
        ia.records_host(m, [0], [34], gt)
    u16 = torch.from_numpy(np.full((1, 4, 4), 33001, np.uint16).view(np.int16))             # u16 bits in a 2-byte tensor
    rec, regular = ia.records_host(m, [0], [33], u16, 1)
    assert rec[0].tolist() == [0, 16, 0, 33001, 16, 16, 0, 7] and regular[0, 7] == 1
    with pytest.raises(lib.PfError, match='runs on the GPU'):
        ia.InstanceAP(device='cpu')
    seg = np.zeros((2, 4, 6), np.int64)
    seg[0, 0] = 13 * 1000 + 2          # car
    seg[0, 1] = 11 * 1000 + 1          # person
    seg[0, 2] = 8                      # stuff
    seg[1, 3] = 18 * 1000 + 7          # bicycle
    seg[1, 0] = 10 * 1000 + 1          # not a thing class
    masks, image, labels, scores = ia.masks_from_id_map(torch.from_numpy(seg), 'trainid')
    assert image.tolist() == [0, 0, 1] and labels.tolist() == [24, 26, 33] and scores.tolist() == [1.0] * 3 and scores.dtype == torch.float64
    assert masks.dtype == torch.uint8 and masks[0].nonzero()[:, 0].unique().tolist() == [1] and int(masks.sum()) == 18
    ids = np.where(seg >= 1000, np.array([0] * 10 + [23, 24, 25, 26, 27, 28, 31, 32, 33])[np.minimum(seg // 1000, 18)] * 1000 + seg % 1000, seg)
    masks2, image2, labels2, _ = ia.masks_from_id_map(ids, 'cityscapes')
    assert image2.tolist() == [0, 0, 1] and labels2.tolist() == [24, 26, 33] and torch.equal(masks2, masks)
    assert ia.masks_from_id_map(np.zeros((4, 6), np.int64))[0].shape == (0, 4, 6)


def test_the_slot_of_a_value_without_a_gpu():
    import ctypes
    from panoptic_forecasting_amd import lib
    L = lib.load()
    slot = ctypes.c_int()
    want = {(26001, 26): 1, (26000, 26): 0, (26999, 26): 999, (26, 26): 1000, (0, 26): 1001, (6, 26): 1001, (7, 26): -1, (29, 26): 1001,
            (29001, 26): -1, (27001, 26): -1, (24, 26): -1, (33999, 33): 999, (65535, 33): -1, (1000, 26): -1, (26001, 7): -1, (30, 24): 1001}
    for (value, label), s in want.items():
        assert L.pf_debug_ap_slot(value, label, ctypes.byref(slot)) == 0 and slot.value == s, (value, label)
    assert L.pf_debug_ap_slot(65536, 26, ctypes.byref(slot)) == -1 and L.pf_debug_ap_slot(5, 34, ctypes.byref(slot)) == -1
    assert L.pf_ap_chunk_pixels() == 16384
