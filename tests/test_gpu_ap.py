"""Instance AP on the device: pf_ap_accumulate / instance_ap.InstanceAP (csrc/ap_kernels.hip) against instance_ap.records_host
(records: integers, equal) and tests/ap_ref64.py (the meter's result: equal bits)."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import ap_ref64 as R
import ap_scenes as S

pytestmark = pytest.mark.gpu
GT_KINDS = ('u16', 'i32', 'i64')
CHUNK = 16384                                  # pf_ap_chunk_pixels(): checked below, the shapes are written out from it
# name -> ((B, H, W), seed, P)
SHAPES = {'smallest': ((1, 1, 1), 1, 2), 'all head and tail': ((2, 3, 5), 2, 5), 'odd width': ((1, 7, 33), 3, 6),
          'exact trips': ((3, 16, 64), 4, 12), 'chunk - 1': ((2, 127, 129), 5, 8), 'chunk': ((2, 128, 128), 6, 8),
          'chunk + 1': ((2, 5, 3277), 7, 8), 'several chunks': ((2, 200, 333), 8, 12)}
MIN_REGION = 3
_REF = {}


def reference(name):
    """(gt, masks, image, labels, scores, rec, gt_regular) of a named case: computed once, shared, read-only."""
    if name not in _REF:
        from panoptic_forecasting_amd import instance_ap as ia
        shape, seed, p = SHAPES[name]
        gt, masks, image, labels, scores = S.random_scene(shape, seed, p)
        rec, regular = ia.records_host(masks, image, labels, gt, MIN_REGION)
        out = (gt, masks, image, labels, scores, rec.numpy(), regular.numpy())
        for a in out:
            a.setflags(write=False)
        _REF[name] = out
    return _REF[name]


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()
    return t if dtype is None else t.to(dtype)


def dev_gt(a, kind='u16'):
    """An instance map on the device: u16 travels as a 2-byte integer tensor with the same bits."""
    a = np.array(a)
    if kind == 'u16':
        return torch.from_numpy(a.astype(np.uint16).view(np.int16)).cuda()
    return torch.from_numpy(a).to('cuda', torch.int32 if kind == 'i32' else torch.int64)


def bits(x):
    return struct.pack('<d', float(x))


def same_ap(a, b):
    return len(a) == len(b) and all(bits(x) == bits(y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


def run(masks, image, labels, scores, gt, meter=None, min_region=MIN_REGION, **kw):
    """device tensors -> (meter, rec, gt_regular as numpy)"""
    from panoptic_forecasting_amd import instance_ap as ia
    m = meter or ia.InstanceAP(min_region)
    rec, regular = m.update(masks, image, labels, scores, gt, **kw)
    return m, rec.cpu().numpy(), regular.cpu().numpy()


def test_the_chunk_constant_is_the_one_the_shapes_were_written_for():
    from panoptic_forecasting_amd import lib
    assert lib.load().pf_ap_chunk_pixels() == CHUNK
    assert 127 * 129 == CHUNK - 1 and 128 * 128 == CHUNK and 5 * 3277 == CHUNK + 1 and 200 * 333 > 4 * CHUNK


@pytest.mark.parametrize('name', list(SHAPES))
def test_records_equal_the_host_for_every_gt_kind_and_the_result_the_restatement(name):
    gt, masks, image, labels, scores, want, want_regular = reference(name)
    m, i, l, s = dev(masks), dev(image), dev(labels), dev(scores)
    for kind in GT_KINDS:
        meter, rec, regular = run(m, i, l, s, dev_gt(gt, kind))
        assert np.array_equal(rec, want), (kind, np.argwhere(rec != want)[:8].tolist())
        assert np.array_equal(regular, want_regular), kind
    res = meter.result()
    ref = R.evaluate(S.per_image(masks, image, labels, scores, gt), MIN_REGION)
    assert same_ap(res['ap'], ref['ap']) and bits(res['allAp']) == bits(ref['allAp']) and bits(res['allAp50%']) == bits(ref['allAp50%'])
    if name == 'several chunks':
        assert (want[:, 0] == 0).sum() >= 6 and (want[:, 4] > 0).sum() >= 4 and want_regular.sum() >= 4 and 0 < res['allAp'] <= 1


def test_the_hand_scene_at_every_min_region_and_bool_masks():
    masks, image, labels, scores, gt, notes = S.hand_scene()
    from panoptic_forecasting_amd import instance_ap as ia
    for min_region in (1, 3, 100):
        want, want_regular = ia.records_host(masks, image, labels, gt, min_region)
        meter, rec, regular = run(dev(masks != 0), dev(image), dev(labels), dev(scores), dev_gt(gt), min_region=min_region)
        assert np.array_equal(rec, want.numpy()) and np.array_equal(regular, want_regular.numpy()), min_region
        ref = R.evaluate(S.per_image(masks, image, labels, scores, gt), min_region)
        assert same_ap(meter.result()['ap'], ref['ap']), min_region
    assert rec[notes['small group']].tolist() == [0, 25, 20, 33, 10, 10, 0, 7]


def test_every_slot_of_a_label_and_ties_go_to_the_smaller_value():
    """One 128x128 image of 16-pixel runs walking the group and all 1000 instances of car in a shuffled order; a mask takes the
    same 8 pixels of every run: every slot ties, the group (the smallest value) is best.  A second mask leaves the group out:
    instance 0 is best."""
    rng = np.random.default_rng(11)
    values = np.array([26] + [26000 + k for k in range(1000)])[rng.permutation(1001)]
    gt = np.full(128 * 128, 7, np.int64)
    gt[:1001 * 16] = np.repeat(values, 16)
    m = np.zeros((2, 128 * 128), np.uint8)
    m[:, :1001 * 16] = np.tile(np.repeat([0, 1, 0], [4, 8, 4]), 1001)
    m[1][gt == 26] = 0
    from panoptic_forecasting_amd import instance_ap as ia
    image, labels = np.zeros(2, np.int32), np.full(2, 26, np.int32)
    want, want_regular = ia.records_host(m.reshape(2, 128, 128), image, labels, gt.reshape(1, 128, 128), 17)
    assert want[0].tolist() == [0, 8008, 8 + 8 + 8000, 26, 8, 16, 0, 2] and want[1].tolist() == [0, 8000, 8000, 26000, 8, 16, 0, 2]
    for kind in GT_KINDS:
        _, rec, regular = run(dev(m.reshape(2, 128, 128)), dev(image), dev(labels), dev(np.ones(2)), dev_gt(gt.reshape(1, 128, 128), kind), min_region=17)
        assert np.array_equal(rec, want.numpy()) and regular.tolist() == [[0] * 8], kind
        _, _, regular = run(dev(m.reshape(2, 128, 128)), dev(image), dev(labels), dev(np.ones(2)), dev_gt(gt.reshape(1, 128, 128), kind), min_region=16)
        assert regular.tolist() == [[0, 0, 1000, 0, 0, 0, 0, 0]], kind


@pytest.mark.parametrize('name', ['odd width', 'several chunks'])
def test_a_mask_stack_one_byte_into_its_buffer(name):
    gt, masks, image, labels, scores, want, want_regular = reference(name)
    parent = torch.zeros(1 + masks.size, dtype=torch.uint8, device='cuda')
    parent[1:] = dev(masks).reshape(-1)
    view = parent[1:].view(masks.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 1
    for kind in GT_KINDS:
        _, rec, regular = run(view, dev(image), dev(labels), dev(scores), dev_gt(gt, kind))
        assert np.array_equal(rec, want) and np.array_equal(regular, want_regular), kind


def test_no_masks_no_images():
    from panoptic_forecasting_amd import instance_ap as ia
    gt, masks, image, labels, scores, want, want_regular = reference('exact trips')
    z = lambda dt: torch.zeros(0, dtype=dt, device='cuda')
    m = ia.InstanceAP(MIN_REGION)
    rec, regular = m.update(dev(masks[:0]), z(torch.int32), z(torch.int32), z(torch.float64), dev_gt(gt))
    assert rec.shape == (0, 8) and np.array_equal(regular.cpu().numpy(), want_regular)
    res = m.result()
    assert all(x == 0.0 or x != x for row in res['ap'] for x in row) and res['allAp'] == 0.0
    none = ia.InstanceAP(MIN_REGION)
    rec, regular = none.update(dev(masks[:0]), z(torch.int32), z(torch.int32), z(torch.float64), dev_gt(gt[:0]))
    assert none._ws is None and rec.shape == (0, 8) and regular.shape == (0, 8) and none.status() == 0
    assert none.result()['allAp'] != none.result()['allAp']
    orphan = ia.InstanceAP(MIN_REGION)                       # masks and no image: every index is out of range
    rec, _ = orphan.update(dev(masks), dev(image), dev(labels), dev(scores), dev_gt(gt[:0]))
    assert (rec[:, 0] == 3).all() and orphan.status() == 2


def test_an_images_records_do_not_depend_on_its_batch_or_on_how_its_masks_are_split():
    from panoptic_forecasting_amd import instance_ap as ia
    gt, masks, image, labels, scores, want, want_regular = reference('exact trips')
    ref = R.evaluate(S.per_image(masks, image, labels, scores, gt), MIN_REGION)
    g = dev_gt(gt)
    alone = ia.InstanceAP(MIN_REGION)
    for b in range(3):                                       # every image alone: its masks' image index is 0
        sel = np.nonzero(image == b)[0]
        _, rec, regular = run(dev(masks[sel]), dev(np.zeros(len(sel), np.int32)), dev(labels[sel]), dev(scores[sel]), g[b:b + 1], meter=alone)
        assert np.array_equal(rec[:, :6], want[sel][:, :6]) and np.array_equal(rec[:, 7], want[sel][:, 7]) and (rec[:, 6] == 0).all(), b
        assert np.array_equal(regular[0], want_regular[b]), b
    assert same_ap(alone.result()['ap'], ref['ap'])
    split = ia.InstanceAP(MIN_REGION)                        # the masks of the batch over two updates
    half = len(masks) // 2
    _, rec_a, regular_a = run(dev(masks[:half]), dev(image[:half]), dev(labels[:half]), dev(scores[:half]), g, meter=split)
    _, rec_b, regular_b = run(dev(masks[half:]), dev(image[half:]), dev(labels[half:]), dev(scores[half:]), g, meter=split, new_images=False)
    assert np.array_equal(np.concatenate([rec_a, rec_b]), want) and np.array_equal(regular_a, want_regular) and np.array_equal(regular_b, want_regular)
    assert same_ap(split.result()['ap'], ref['ap'])
    assert split.records()[1].shape == (3, 8)               # the regions of the batch are counted once
    twice = ia.InstanceAP(MIN_REGION)                        # the same batch as two batches of new images: twice the regions
    run(dev(masks), dev(image), dev(labels), dev(scores), g, meter=twice)
    run(dev(masks), dev(image), dev(labels), dev(scores), g, meter=twice)
    rec2, regular2, scores2 = twice.records()
    assert regular2.shape == (6, 8) and rec2[len(masks):, 6].tolist() == (image + 3).tolist()
    both = R.evaluate(S.per_image(masks, image, labels, scores, gt) * 2, MIN_REGION)
    assert same_ap(twice.result()['ap'], both['ap'])


FLAGGED = [(65536, 'i32'), (-1, 'i32'), (65536, 'i64'), (-1, 'i64'), (2 ** 33 + 5, 'i64')]


@pytest.mark.parametrize('bad,kind', FLAGGED)
def test_a_value_out_of_range_flags_its_image_only_and_is_sticky(bad, kind):
    from panoptic_forecasting_amd import instance_ap as ia, lib
    gt, masks, image, labels, scores, want, want_regular = reference('exact trips')
    want, want_regular = want.copy(), want_regular.copy()
    hit = image == 1
    want[hit, 0], want[hit, 1:6] = 3, [0, 0, -1, 0, 0]
    want_regular[1] = 0
    for at in ((1, 15, 63), (1, 0, 0), (1, 7, 30)):          # the last pixel, the first, mid-image
        g = dev_gt(gt, kind)
        g[at] = bad
        m, rec, regular = run(dev(masks), dev(image), dev(labels), dev(scores), g)
        assert np.array_equal(rec, want) and np.array_equal(regular, want_regular), at
        with pytest.raises(lib.PfError, match='PF_AP_STATUS_VALUE'):
            m.result()
        assert m.status() == 1
        run(dev(masks), dev(image), dev(labels), dev(scores), dev_gt(gt, kind), meter=m)      # a clean update: the bit stays
        assert m.status() == 1
        assert m.reset().status() == 0 and m.records()[0].shape == (0, 8)
    odd = dev_gt(gt[:1, :3, :5], kind).contiguous()          # head / tail lanes only
    odd[0, 2, 4] = bad
    m, rec, regular = run(dev(masks[:2, :3, :5]).contiguous(), dev(np.zeros(2, np.int32)), dev(labels[:2]), dev(scores[:2]), odd)
    assert m.status() == 1 and int(regular.sum()) == 0 and (rec[:, 0] >= 2).all()


def test_a_bad_index_flags_its_prediction_only_and_is_sticky():
    from panoptic_forecasting_amd import instance_ap as ia, lib
    gt, masks, image, labels, scores, want, want_regular = reference('exact trips')
    for column, bad in (('image', 3), ('image', -1), ('label', 34), ('label', -5)):
        i, l, w = image.copy(), labels.copy(), want.copy()
        k = int(np.nonzero(want[:, 0] == 0)[0][0])
        if column == 'image':
            i[k] = bad
            w[k] = [3, 0, 0, -1, 0, 0, bad, -1]
        else:
            l[k] = bad
            w[k] = [3, 0, 0, -1, 0, 0, image[k], -1]
        m, rec, regular = run(dev(masks), dev(i), dev(l), dev(scores), dev_gt(gt))
        assert np.array_equal(rec, w) and np.array_equal(regular, want_regular), (column, bad)
        with pytest.raises(lib.PfError, match='PF_AP_STATUS_INDEX'):
            m.result()
        assert m.status() == 2 and m.reset().status() == 0


def test_update_does_not_synchronise_and_a_captured_update_replays_to_the_eager_records():
    from panoptic_forecasting_amd import instance_ap as ia, lib
    gt, masks, image, labels, scores, want, want_regular = reference('chunk + 1')
    m, i, l, s, g = dev(masks), dev(image), dev(labels), dev(scores), dev_gt(gt)
    meter = ia.InstanceAP(MIN_REGION)
    out = (torch.full((len(masks), 8), -7, dtype=torch.int32, device='cuda'), torch.full((len(gt), 8), -7, dtype=torch.int32, device='cuda'))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        meter.update(m, i, l, s, g, out=out)                 # first call: allocates the workspace too
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert np.array_equal(out[0].cpu().numpy(), want)
    meter.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        meter.update(m, i, l, s, g, out=out)
    for rep in range(3):
        out[0].fill_(-7), out[1].fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out[0].cpu().numpy(), want) and np.array_equal(out[1].cpu().numpy(), want_regular), rep
    ref = R.evaluate(S.per_image(masks, image, labels, scores, gt), MIN_REGION)
    assert same_ap(meter.result()['ap'], ref['ap'])
    big = dev(np.concatenate([masks, masks]))
    with pytest.raises(lib.PfError, match='after a graph capture'):
        meter.update(big, torch.cat([i, i]), torch.cat([l, l]), torch.cat([s, s]), g)
    meter.update(m[:1], i[:1], l[:1], s[:1], g)              # fewer masks still fit


def test_arguments():
    from panoptic_forecasting_amd import instance_ap as ia, lib
    with pytest.raises(lib.PfError, match='runs on the GPU .* records_host'):
        ia.InstanceAP(device='cpu')
    m = ia.InstanceAP()
    z = lambda *s, dt=torch.uint8, d='cuda': torch.zeros(*s, dtype=dt, device=d)
    i32 = torch.int32
    ok = dict(masks=z(2, 8, 8), mask_image=z(2, dt=i32), labels=z(2, dt=i32), scores=z(2, dt=torch.float32), gt=z(1, 8, 8, dt=torch.int16))
    m.update(**ok)
    for key, value, text in (('masks', z(2, 8, 8, dt=i32), 'u8 or bool'), ('gt', z(1, 8, 9, dt=torch.int16), 'image shape'),
                             ('gt', z(1, 8, 8), 'integer instance map'), ('gt', z(1, 8, 8, dt=torch.float32), 'integer instance map'),
                             ('mask_image', z(2, dt=torch.int64), 'mask_image must be int32'), ('labels', z(3, dt=i32), 'labels must be int32'),
                             ('scores', z(3, dt=torch.float32), 'scores must be'), ('gt', z(1, 8, 8, dt=torch.int16, d='cpu'), 'must live on the GPU'),
                             ('masks', z(2, 8, 16)[:, :, ::2], 'contiguous')):
        with pytest.raises(lib.PfError, match=text):
            m.update(**dict(ok, **{key: value}))
    with pytest.raises(lib.PfError, match='new_images=False'):
        ia.InstanceAP().update(new_images=False, **ok)
    L = lib.load()
    need = ctypes.c_size_t()
    assert L.pf_ap_workspace(2, 1, ctypes.byref(need)) == 0 and need.value >= 256 + 8 * 1001 * 4 + 2 * 1003 * 4
    ws = z(256)
    a = ok['mask_image'].data_ptr()
    call = lambda *args, n=256: L.pf_ap_accumulate(*args, a, a, ws.data_ptr(), n, lib.stream_ptr())
    assert call(None, None, None, 0, None, 0, 0, 8, 8, 100) == 0
    assert call(a, a, a, 2, a, 0, 1, 8, 8, 100) == -2        # PF_EWORKSPACE
    assert call(a, a, a, 2, a, 3, 1, 8, 8, 100) == -1        # PF_EINVAL: gt_kind
    assert call(a, a, a, 2, a, 0, 1, 8, 8, -1) == -1         # min_region
    assert call(a, a, a, 2, a + 4, 2, 1, 8, 8, 100) == -1    # an i64 map at +4
    assert call(a, a, a, 2, a, 0, 1, 32768, 32768, 100, n=1 << 20) == -5   # PF_EUNSUPPORTED: H * W
    torch.cuda.synchronize()
