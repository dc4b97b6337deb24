"""iIoU on the device: pf_iiou_accumulate / semantic_iou.SemanticIoU.update(..., inst=) (csrc/iiou_kernels.hip) against
tests/iiou_ref64.py.  The per-image sums are float64 in a fixed order of operations: every comparison is equality of bits, the
counts are integers and equal."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import conf_ref64 as C
import iiou_ref64 as R
import iiou_scenes as IS

pytestmark = pytest.mark.gpu
PRED_KINDS = {'u8': torch.uint8, 'i32': torch.int32, 'i64': torch.int64}
INST_KINDS = ('u16', 'i32', 'i64')
FMTS = ('trainid', 'cityscapes')
CHUNK = 16384                                  # pf_iiou_chunk_pixels(): checked below, the shapes are written out from it
ORDER_SEED = 3                                 # tests/test_iiou_host.py asserts that the order shows in this input's bits
SHAPES = {'smallest': ((1, 1, 1), 1), 'all head and tail': ((2, 3, 5), 2), 'odd width': ((1, 7, 33), 3), 'exact trips': ((3, 16, 64), 4),
          'chunk - 1': ((2, 127, 129), 5), 'chunk': ((2, 128, 128), 6), 'chunk + 1': ((2, 5, 3277), 7), 'several chunks': ((2, 200, 333), 8)}
_REF = {}


def reference(name, fmt):
    """(pred, inst, per_image, per_image_counts) of a named case in ``fmt``: computed once, shared, read-only."""
    if (name, fmt) not in _REF:
        pred, inst = IS.inst_run_maps(*SHAPES[name])
        pred = IS.in_format(pred, fmt)
        per, counts = R.instance_sums(pred, inst, 19, fmt)
        for a in (pred, inst, per, counts):
            a.setflags(write=False)
        _REF[(name, fmt)] = (pred, inst, per, counts)
    return _REF[(name, fmt)]


def dev(a, dtype=torch.uint8):
    return torch.from_numpy(np.array(a)).to('cuda', dtype)


def dev_inst(a, kind='u16'):
    """An instance map on the device: u16 travels as a 2-byte integer tensor with the same bits."""
    a = np.array(a)
    if kind == 'u16':
        return torch.from_numpy(a.astype(np.uint16).view(np.int16)).cuda()
    return torch.from_numpy(a).to('cuda', torch.int32 if kind == 'i32' else torch.int64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def blocks(b):
    return (torch.full((b, 8, 2), -7.0, dtype=torch.float64, device='cuda'), torch.full((b, 8, 3), -7, dtype=torch.int64, device='cuda'))


def run(pred, inst, fmt='trainid', n_cls=19, meter=None, check=True):
    """pred, inst: device tensors -> (meter, per_image, per_image_counts as numpy); the prediction stands in for the ground truth
    of the confusion call."""
    from panoptic_forecasting_amd import semantic_iou as si
    m = meter or si.SemanticIoU(n_cls, fmt)
    per, counts = blocks(len(pred))
    m.update(pred, pred, inst=inst, per_image_inst=per, per_image_inst_counts=counts)
    if check:
        m.result()
    return m, per.cpu().numpy(), counts.cpu().numpy()


def assert_equals_reference(pred, inst, want, want_counts, fmt='trainid', note=None):
    m, per, counts = run(pred, inst, fmt)
    assert same_bits(per, want), (note, np.argwhere(per != want)[:8].tolist())
    assert np.array_equal(counts, want_counts), (note, np.argwhere(counts != want_counts)[:8].tolist())
    assert same_bits(m.acc_inst.cpu().numpy(), R.running_sum(want)), note
    assert np.array_equal(m.acc_inst_counts.cpu().numpy(), want_counts.sum(0)), note


def test_the_chunk_constant_is_the_one_the_shapes_were_written_for():
    from panoptic_forecasting_amd import lib
    assert lib.load().pf_iiou_chunk_pixels() == CHUNK
    assert 127 * 129 == CHUNK - 1 and 128 * 128 == CHUNK and 5 * 3277 == CHUNK + 1 and 200 * 333 > 4 * CHUNK


@pytest.mark.parametrize('name', list(SHAPES))
def test_sums_equal_the_restatement_for_every_kind_pair_and_format(name):
    for fmt in FMTS:
        pred, inst, want, want_counts = reference(name, fmt)
        preds = {k: dev(pred, dt) for k, dt in PRED_KINDS.items()}
        insts = {k: dev_inst(inst, k) for k in INST_KINDS}
        for pk in PRED_KINDS:
            for ik in INST_KINDS:
                assert_equals_reference(preds[pk], insts[ik], want, want_counts, fmt, (fmt, pk, ik))
    if name == 'several chunks':
        assert want_counts[:, :, 0].min() >= 3 and (want_counts[:, :, 2] > 0).all()      # every class, with hits


def test_every_slot_of_the_table():
    """Two 128x128 images of 4-pixel runs whose ids walk through all 8 x 1000 slots once, in a shuffled order: 4000 instances in
    one chunk - more than a workgroup's table in LDS holds - with k = 0 and k = 999 of every class; half of each run is hit."""
    rng = np.random.default_rng(11)
    slots = rng.permutation(8000)
    inst, pred = np.zeros((2, 4096), np.int64), np.full((2, 4096), 255, np.int64)
    inst[:, :4000] = np.array([IS.THING_LABELS[s // 1000] * 1000 + s % 1000 for s in slots]).reshape(2, 4000)
    pred[:, :4000] = 11 + (slots // 1000).reshape(2, 4000)
    inst = np.repeat(inst, 4, axis=1).reshape(2, 128, 128)
    pred = np.repeat(pred, 4, axis=1)
    pred[:, 0::4], pred[:, 3::4] = 0, 255
    pred = pred.reshape(2, 128, 128)
    want, want_counts = R.instance_sums(pred, inst)
    assert want_counts[:, :, 0].sum() == 8000 and want_counts[:, :, 1].sum() == 32000 and want_counts[:, :, 2].sum() == 16000
    for pk, ik in (('u8', 'u16'), ('i32', 'i32'), ('u8', 'i64')):
        assert_equals_reference(dev(pred, PRED_KINDS[pk]), dev_inst(inst, ik), want, want_counts, note=(pk, ik))


def test_an_instance_spans_chunks_and_runs_do_not_leak_between_images():
    pred, inst = np.full((1, 200, 333), 13, np.int64), np.full((1, 200, 333), 26005, np.int64)
    pred[0, 150:] = 2
    want, want_counts = R.instance_sums(pred, inst)
    assert want_counts[0, 2].tolist() == [1, 66600, 49950] and want[0, 2, 0] == 49950 * (12794.0202738185 / 66600)
    for ik in INST_KINDS:
        assert_equals_reference(dev(pred), dev_inst(inst, ik), want, want_counts, note=ik)
    for shape in ((2, 4, 16), (2, 3, 5), (2, 128, 128)):
        # the last pixel of image 0 and the first of image 1 carry one id, which each image holds nowhere else
        pred, inst = np.full(shape, 11, np.int64), np.full(shape, 24001, np.int64)
        inst[0, -1, -1], inst[1, 0, 0] = 33007, 33007
        pred[0, -1, -1], pred[1, 0, 0] = 18, 18
        n = shape[1] * shape[2]
        want, want_counts = R.instance_sums(pred, inst)
        assert want_counts[:, 7].tolist() == [[1, 1, 1]] * 2 and want_counts[:, 0].tolist() == [[1, n - 1, n - 1]] * 2
        for pk, ik in (('u8', 'u16'), ('i32', 'i32'), ('i64', 'i64')):
            assert_equals_reference(dev(pred, PRED_KINDS[pk]), dev_inst(inst, ik), want, want_counts, note=(shape, pk, ik))


def test_the_device_adds_in_ascending_instance_value():
    pred, inst = IS.many_persons(ORDER_SEED)
    up, counts = R.instance_sums(pred, inst)
    down, _ = R.instance_sums(pred, inst, descending=True)
    assert counts[0, 0, 0] >= 200 and not same_bits(up[0, 0], down[0, 0])
    for pk, ik in (('u8', 'u16'), ('i64', 'i32')):
        assert_equals_reference(dev(pred, PRED_KINDS[pk]), dev_inst(inst, ik), up, counts, note=(pk, ik))


@pytest.mark.parametrize('fmt', FMTS)
def test_misaligned_base_pointers(fmt):
    """[1:] of a flat parent of 1 + 2*64*100 elements: the base is one element past an aligned address - 1 byte for u8, 2 for
    u16, 4 for i32, 8 for i64; H*W = 6400 keeps image 1 as far off as image 0.  Both maps shifted, and either one alone: where no
    head aligns both, the map left misaligned is read by element loads."""
    pred, inst = IS.inst_run_maps((2, 64, 100), 9)
    pred = IS.in_format(pred, fmt)
    want, want_counts = R.instance_sums(pred, inst, 19, fmt)

    def shifted(t):
        parent = torch.zeros(1 + t.numel(), dtype=t.dtype, device='cuda')
        parent[1:] = t.reshape(-1)
        view = parent[1:].view(t.shape)
        assert view.is_contiguous() and view.data_ptr() % 16 == parent.element_size()
        return view

    for pk, pdt in PRED_KINDS.items():
        for ik in INST_KINDS:
            p, i = dev(pred, pdt), dev_inst(inst, ik)
            for pp, ii in ((shifted(p), shifted(i)), (shifted(p), i), (p, shifted(i))):
                assert_equals_reference(pp, ii, want, want_counts, fmt, (pk, ik, pp.data_ptr() % 16, ii.data_ptr() % 16))


def test_an_images_sums_do_not_depend_on_its_batch():
    from panoptic_forecasting_amd import semantic_iou as si
    pred, _, inst = IS.make_scenes(n=5)
    want, want_counts = R.instance_sums(pred, inst)
    assert (want_counts[:, :, 0].sum(1) > 0).sum() >= 4
    p, i = dev(pred), dev_inst(inst)
    m = si.SemanticIoU()
    _, per_a, counts_a = run(p[:3], i[:3], meter=m)
    _, per_b, counts_b = run(p[3:], i[3:], meter=m)                   # a second update of the same meter
    assert same_bits(np.concatenate([per_a, per_b]), want) and np.array_equal(np.concatenate([counts_a, counts_b]), want_counts)
    assert same_bits(m.acc_inst.cpu().numpy(), R.running_sum(want)) and np.array_equal(m.acc_inst_counts.cpu().numpy(), want_counts.sum(0))
    for k in range(5):
        _, alone, counts_alone = run(p[k:k + 1], i[k:k + 1])
        assert same_bits(alone[0], want[k]) and np.array_equal(counts_alone[0], want_counts[k]), k
    res = m.result()
    table = C.confusion(pred, pred)[0]
    ref = R.iiou(table, R.running_sum(want))
    assert res['iIoU']['n'] == ref['n'] > 0 and abs(res['iIoU']['miou'] - ref['miou']) <= 1e-12 * ref['miou']
    assert res['categories']['iiou']['n'] == R.categories(table, R.running_sum(want))['iiou']['n']


FLAGGED = [('inst', 65536, 'i32'), ('inst', -1, 'i32'), ('inst', 65536, 'i64'), ('inst', -1, 'i64'), ('inst', 2 ** 33 + 5, 'i64'),
           ('pred', 256, 'i32'), ('pred', 256, 'i64')]


@pytest.mark.parametrize('which,bad,kind', FLAGGED)
def test_values_out_of_range_set_the_flag(which, bad, kind):
    """The flagged image adds nothing and its blocks are zero, its neighbours still count; result() raises, reset() clears; the
    confusion table of the update is what it is without the instance map."""
    from panoptic_forecasting_amd import lib, semantic_iou as si
    pred, gt, inst = IS.make_scenes(n=3)
    want, want_counts = R.instance_sums(pred, inst)
    want, want_counts = want.copy(), want_counts.copy()
    want[1], want_counts[1] = 0, 0
    wide = torch.int32 if kind == 'i32' else torch.int64
    for at in ((1, 63, 127), (1, 0, 0), (1, 20, 77)):            # the last pixel, the first, mid-image
        p = dev(pred, wide if which == 'pred' else torch.uint8)
        i = dev_inst(inst, kind if which == 'inst' else 'u16')
        (p if which == 'pred' else i)[at] = bad
        m = si.SemanticIoU()
        per, counts = blocks(3)
        m.update(p, dev(gt), inst=i, per_image_inst=per, per_image_inst_counts=counts)
        with pytest.raises(lib.PfError, match='PF_IIOU_STATUS_VALUE'):
            m.result()
        assert m.status() == 1
        assert same_bits(per.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), want_counts)
        assert same_bits(m.acc_inst.cpu().numpy(), R.running_sum(want)) and np.array_equal(m.acc_inst_counts.cpu().numpy(), want_counts.sum(0))
        plain = si.SemanticIoU().update(p, dev(gt))
        assert torch.equal(m.acc, plain.acc)
        assert m.reset().status() == 0 and float(m.acc_inst.abs().sum()) == 0 and int(m.acc_inst_counts.abs().sum()) == 0
        m.update(dev(pred), dev(gt), inst=dev_inst(inst))
        m.result()
        assert same_bits(m.acc_inst.cpu().numpy(), R.running_sum(R.instance_sums(pred, inst)[0]))
    odd_p = dev(pred[:1, :3, :5], wide if which == 'pred' else torch.uint8).contiguous()     # head / tail lanes only
    odd_i = dev_inst(inst[:1, :3, :5], kind if which == 'inst' else 'u16').contiguous()
    (odd_p if which == 'pred' else odd_i)[0, 2, 4] = bad
    m = si.SemanticIoU().update(odd_p, odd_p, inst=odd_i)
    assert m.status() == 1 and float(m.acc_inst.abs().sum()) == 0


def test_arguments_dtypes_shapes_and_mixed_updates():
    from panoptic_forecasting_amd import lib, semantic_iou as si
    m = si.SemanticIoU()
    z = lambda *s, dt=torch.uint8, d='cuda': torch.zeros(*s, dtype=dt, device=d)
    m.update(z(0, 8, 8), z(0, 8, 8), inst=z(0, 8, 8, dt=torch.int16))
    assert m._ws_inst is None and m.status() == 0
    L = lib.load()
    ws = z(256)
    a, c = m.acc_inst.data_ptr(), m.acc_inst_counts.data_ptr()
    call = lambda *args: L.pf_iiou_accumulate(*args, a, c, None, None, ws.data_ptr(), 256, lib.stream_ptr())
    assert call(None, 0, None, 0, 0, 19, 0, 8, 8) == 0
    need = ctypes.c_size_t()
    assert L.pf_iiou_workspace(2, ctypes.byref(need)) == 0 and need.value >= 256 + 2 * 64000
    assert call(a, 0, a, 0, 0, 19, 2, 8, 8) == -2               # PF_EWORKSPACE
    assert call(a, 3, a, 0, 0, 19, 2, 8, 8) == -1               # PF_EINVAL
    assert call(a, 0, a, 3, 0, 19, 2, 8, 8) == -1
    assert call(a, 0, a, 0, 0, 20, 2, 8, 8) == -1
    assert call(a + 4, 2, a, 0, 0, 19, 2, 8, 8) == -1           # an i64 prediction at +4
    assert call(a, 0, a + 4, 2, 0, 19, 2, 8, 8) == -1           # an i64 instance map at +4
    assert call(a, 0, a + 1, 0, 0, 19, 2, 8, 8) == -1           # a u16 instance map at +1
    torch.cuda.synchronize()
    assert float(m.acc_inst.abs().sum()) == 0
    with pytest.raises(lib.PfError, match='must live on the GPU'):
        m.update(z(1, 8, 8), z(1, 8, 8), inst=z(1, 8, 8, dt=torch.int16, d='cpu'))
    with pytest.raises(lib.PfError, match='integer instance map'):
        m.update(z(1, 8, 8), z(1, 8, 8), inst=z(1, 8, 8, dt=torch.float32))
    with pytest.raises(lib.PfError, match='integer instance map'):
        m.update(z(1, 8, 8), z(1, 8, 8), inst=z(1, 8, 8, dt=torch.float16))
    with pytest.raises(lib.PfError, match='integer instance map'):
        m.update(z(1, 8, 8), z(1, 8, 8), inst=z(1, 8, 8, dt=torch.bool))
    with pytest.raises(lib.PfError, match='integer instance map'):
        m.update(z(1, 8, 8), z(1, 8, 8), inst=z(1, 8, 8))                      # u8 cannot hold an instance id
    with pytest.raises(lib.PfError, match='shape of pred'):
        m.update(z(1, 8, 8), z(1, 8, 8), inst=z(1, 8, 9, dt=torch.int16))
    with pytest.raises(lib.PfError, match='contiguous'):
        m.update(z(1, 8, 8), z(1, 8, 8), inst=z(1, 8, 16, dt=torch.int16)[:, :, ::2])
    with pytest.raises(lib.PfError, match='per_image_inst'):
        m.update(z(1, 8, 8), z(1, 8, 8), inst=z(1, 8, 8, dt=torch.int16), per_image_inst=z(1, 8, 3, dt=torch.float64))
    with pytest.raises(lib.PfError, match='per_image_inst_counts'):
        m.update(z(1, 8, 8), z(1, 8, 8), inst=z(1, 8, 8, dt=torch.int16), per_image_inst_counts=z(1, 8, 3, dt=torch.float64))
    with pytest.raises(lib.PfError, match='need inst'):
        m.update(z(1, 8, 8), z(1, 8, 8), per_image_inst=z(1, 8, 2, dt=torch.float64))
    assert m._updates == [0, 0]
    m.update(z(1, 8, 8), z(1, 8, 8), inst=z(1, 8, 8, dt=torch.int16))
    assert 'iIoU' in m.result()
    m.update(z(1, 8, 8), z(1, 8, 8))
    with pytest.raises(lib.PfError, match='with an instance map and 1 without'):
        m.result()
    assert 'iIoU' not in m.reset().update(z(1, 8, 8), z(1, 8, 8)).result()


def test_two_meters_give_equal_bits_and_update_does_not_synchronise():
    from panoptic_forecasting_amd import semantic_iou as si
    pred, gt, inst = IS.make_scenes(n=8)
    p, g, i = dev(pred), dev(gt), dev_inst(inst)
    one, two = si.SemanticIoU(), si.SemanticIoU()
    (pa, ca), (pb, cb) = blocks(8), blocks(8)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        one.update(p, g, inst=i, per_image_inst=pa, per_image_inst_counts=ca)           # first call: allocates the workspaces too
        two.update(p, g, inst=i, per_image_inst=pb, per_image_inst_counts=cb)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    one.result(), two.result()
    assert torch.equal(one.acc_inst.view(torch.int64), two.acc_inst.view(torch.int64)) and torch.equal(pa.view(torch.int64), pb.view(torch.int64))
    assert torch.equal(one.acc_inst_counts, two.acc_inst_counts) and torch.equal(ca, cb) and torch.equal(one.acc, two.acc)
    assert same_bits(pa.cpu().numpy(), R.instance_sums(pred, inst)[0])


def test_graph_replays_equal_eager_and_the_workspace_may_not_grow_around_a_capture(monkeypatch):
    """One update with an instance map captured after a warm-up update at that B, replayed five times with the accumulators
    re-zeroed in between: every replay gives the eager bits (the call zeroes its tables itself, with kernel nodes)."""
    from panoptic_forecasting_amd import lib, semantic_iou as si
    pred, gt, inst = IS.make_scenes(n=4)
    p, g, i = dev(pred), dev(gt, torch.int32), dev_inst(inst)
    eager = si.SemanticIoU().update(p, g, inst=i)
    eager.result()
    assert float(eager.acc_inst.sum()) > 0
    m = si.SemanticIoU()
    per, counts = blocks(4)
    m.update(p, g, inst=i, per_image_inst=per, per_image_inst_counts=counts)      # sizes both workspaces outside the capture
    m.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.update(p, g, inst=i, per_image_inst=per, per_image_inst_counts=counts)
    for rep in range(5):
        m.acc.zero_(), m.acc_inst.zero_(), m.acc_inst_counts.zero_()
        per.fill_(-7), counts.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(m.acc_inst.view(torch.int64), eager.acc_inst.view(torch.int64)) and torch.equal(m.acc, eager.acc), rep
        assert torch.equal(m.acc_inst_counts, eager.acc_inst_counts) and torch.equal(counts.sum(0), eager.acc_inst_counts), rep
        assert same_bits(per.cpu().numpy(), R.instance_sums(pred, inst)[0]), rep
    m.result()
    big = [dev(np.concatenate([x, x])) for x in (pred, gt)] + [dev_inst(np.concatenate([inst, inst]))]
    with pytest.raises(lib.PfError, match='after a graph capture'):
        m.update(big[0], big[1], inst=big[2])          # B = 8 would replace the captured workspaces
    m.update(p[:1], g[:1], inst=i[:1])                 # a smaller batch still fits
    m.result()
    fresh = si.SemanticIoU().update(p[:1], g[:1], inst=i[:1])
    fresh.result()
    grown = si.SemanticIoU().update(p, g)              # the confusion workspace holds B = 4, the iIoU workspace does not exist
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)   # no capture is begun only to be abandoned
    with pytest.raises(lib.PfError, match='during a graph capture'):
        fresh.update(p, g, inst=i)
    with pytest.raises(lib.PfError, match='iiou workspace .* during a graph capture'):
        grown.update(p, g, inst=i)


def _clean_env():
    return {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}


@pytest.mark.parametrize('fmt', FMTS)
def test_driver_device_matcher_gives_the_host_file(tmp_path, fmt):
    from panoptic_forecasting_amd import eval_semantic
    pred, gt, inst = IS.make_scenes(n=3, h=32, w=48, seed=9)
    flags = IS.write_tree(str(tmp_path), pred, gt, inst, fmt)
    host, device = str(tmp_path / 'host.json'), str(tmp_path / 'device.json')
    eval_semantic.run(eval_semantic.parse_args(flags + ['--results_file', host, '--matcher', 'host']))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'panoptic-forecasting_amd', 'eval_semantic.py')] + flags +
                       ['--results_file', device, '--batch_size', '2', '--num_workers', '2'], capture_output=True, text=True, timeout=300,
                       env=_clean_env())
    assert r.returncode == 0, r.stderr[-3000:]
    with open(host) as f:
        a = json.load(f)
    with open(device) as f:
        b = json.load(f)
    assert a == b and a['iIoU']['n'] > 0 and a['categories']['iiou'] is not None
    assert 'iIoU' in r.stdout and 'vehicle' in r.stdout


def test_driver_two_gloo_ranks_equal_the_single_process_file(tmp_path):
    """Two ranks sharing the GPU over gloo, device matcher: the per-image pairs are added in one order, so the file is the
    single process's."""
    import iiou_eval_worker
    from panoptic_forecasting_amd import eval_semantic
    pred, gt, inst = IS.make_scenes(n=5, h=32, w=48, seed=9)
    flags = IS.write_tree(str(tmp_path), pred, gt, inst, 'cityscapes')
    one, two = str(tmp_path / 'one.json'), str(tmp_path / 'two.json')
    eval_semantic.run(eval_semantic.parse_args(flags + ['--results_file', one]))
    iiou_eval_worker.spawn_two(flags + ['--results_file', two, '--batch_size', '2'])
    with open(one) as f:
        a = json.load(f)
    with open(two) as f:
        b = json.load(f)
    assert a == b and a['iIoU']['n'] > 0


def test_an_update_without_an_instance_map_is_what_it_was():
    from panoptic_forecasting_amd import semantic_iou as si
    pred, gt, _ = IS.make_scenes(n=3)
    m = si.SemanticIoU().update(dev(pred), dev(gt))
    res = m.result()
    assert m._ws_inst is None and sorted(res) == ['All', 'MO', 'Stuff', 'per_class', 'pixel_acc']
    assert np.array_equal(m.acc.cpu().numpy(), C.confusion(pred, gt)[0])
    assert float(m.acc_inst.abs().sum()) == 0 and int(m.acc_inst_counts.abs().sum()) == 0
