"""Panoptic quality on the device: pf_pq_accumulate / pq.PanopticQuality (csrc/pq_kernels.hip) against tests/pq_ref64.py.

Counts (TP, FP, FN) must be equal; sum_iou within 1e-12 relative.  The bound is derived, not measured: each IoU is one fp64
division, off by at most 2 ulp even if the build's division is not correctly rounded, a class adds fewer than 1000 of them per
call, so any order of addition is within 1000 * 2^-52 = 2.2e-13 of the exact sum; 1e-12 leaves a factor of four."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import pq_ref64 as R
import pq_scenes as S

pytestmark = pytest.mark.gpu
REL = 1e-12
DTYPES = {'i32': torch.int32, 'i64': torch.int64}


def assert_acc(got, want, what=''):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(got[..., 1:], want[..., 1:]), '%s counts differ at %s' % (what, np.argwhere(got[..., 1:] != want[..., 1:])[:8].tolist())
    err = np.abs(got[..., 0] - want[..., 0])
    assert (err <= REL * np.abs(want[..., 0])).all(), '%s sum_iou off by %g' % (what, err.max())


def dev(a, dtype=torch.int64):
    return torch.from_numpy(np.array(a)).to('cuda', dtype)


def run(pred, gt, fmt='trainid', crowd=True, n_cls=19, pdt=torch.int32, gdt=torch.int32):
    """-> (acc, per_image) numpy, after result() found a clean status word."""
    from panoptic_forecasting_amd import pq
    m = pq.PanopticQuality(n_cls, fmt, crowd)
    per = torch.full((len(pred), n_cls, 4), -7.0, dtype=torch.float64, device='cuda')
    m.update(dev(pred, pdt), dev(gt, gdt), per_image=per)
    m.result()
    return m.acc.cpu().numpy(), per.cpu().numpy()


@pytest.fixture(scope='module')
def scenes():
    preds, gts = S.make_scenes()
    preds.setflags(write=False)
    gts.setflags(write=False)
    return preds, gts, R.accumulate(preds, gts, 19, 'trainid', True)


def striped(h, w, modulus):
    """pred = pixel index % modulus + 11000 against two stripes of ground truth (an instance above, car crowd below)."""
    idx = np.arange(h * w, dtype=np.int64).reshape(1, h, w)
    gt = np.where(idx < h * w // 2, 12001, 13)
    return idx % modulus + 11000, gt


@pytest.mark.parametrize('pdt', ['i32', 'i64'])
@pytest.mark.parametrize('gdt', ['i32', 'i64'])
def test_hand_made_scenes_both_formats_every_dtype(pdt, gdt):
    cases = S.hand_scenes()
    preds, gts = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
    for crowd in (True, False):
        want, want_per, _ = R.accumulate(preds, gts, 19, 'trainid', crowd)
        for i, (name, _, _, expect) in enumerate(cases):
            for (cr, c), row in expect.items():
                if cr == crowd:
                    assert tuple(want_per[i, c, 1:].astype(int)) == row, name
        for fmt in ('trainid', 'cityscapes'):
            p, g = (preds, gts) if fmt == 'trainid' else (R.to_cityscapes(preds), R.to_cityscapes(gts))
            acc, per = run(p, g, fmt, crowd, pdt=DTYPES[pdt], gdt=DTYPES[gdt])
            assert_acc(per, want_per, '%s crowd=%s per_image' % (fmt, crowd))
            assert_acc(acc, want, '%s crowd=%s' % (fmt, crowd))


@pytest.mark.parametrize('fmt,crowd,n_cls', [('trainid', True, 19), ('cityscapes', True, 19), ('trainid', False, 19), ('cityscapes', True, 11)])
def test_generated_scenes(scenes, fmt, crowd, n_cls):
    preds, gts, ref = scenes
    want, want_per, _ = ref if (crowd, n_cls) == (True, 19) else R.accumulate(preds, gts, n_cls, 'trainid', crowd)
    p, g = (preds, gts) if fmt == 'trainid' else (R.to_cityscapes(preds), R.to_cityscapes(gts))
    acc, per = run(p, g, fmt, crowd, n_cls, pdt=torch.int64)
    print('max |d sum_iou| = %.3g' % np.abs(acc[:, 0] - want[:, 0]).max())
    assert_acc(per, want_per, 'per_image')
    assert_acc(acc, want, 'acc')


def test_one_call_equals_three_calls_bit_for_bit_and_runs_repeat(scenes):
    from panoptic_forecasting_amd import pq
    preds, gts, ref = scenes
    p, g = dev(preds, torch.int32), dev(gts, torch.int64)
    one = pq.PanopticQuality().update(p, g)
    again = pq.PanopticQuality().update(p, g)
    three = pq.PanopticQuality()
    for i in range(0, 24, 8):
        three.update(p[i:i + 8], g[i:i + 8])
    one.result(), three.result(), again.result()
    assert torch.equal(one.acc, three.acc) and torch.equal(one.acc, again.acc)
    assert_acc(one.acc.cpu().numpy(), ref[0])


def test_large_segments_span_every_workgroup():
    """256x512: 16 count workgroups, the bands and the big rectangles lie in all of them: several LDS tables flush into one
    image table."""
    preds, gts = S.make_scenes(n=1, h=256, w=512, seed=11)
    want, want_per, _ = R.accumulate(preds, gts)
    assert want[:, 1].sum() >= 4
    acc, per = run(preds, gts, pdt=torch.int64, gdt=torch.int32)
    assert_acc(per, want_per)
    assert_acc(acc, want)


def test_more_pairs_than_an_lds_table_holds():
    """64x128 = one count workgroup; 6000 distinct pairs: the LDS table (1024 slots) overflows into the image's table
    (pf_pq_table_slots() = 8192 > 6000), and every count must still be exact."""
    from panoptic_forecasting_amd import lib
    pred, gt = striped(64, 128, 3000)
    n_pairs = len(np.unique(gt.ravel() * 65536 + pred.ravel()))
    assert 1024 * 4 < n_pairs == 6000 < lib.load().pf_pq_table_slots()
    for crowd in (True, False):
        want, want_per, excused = R.accumulate(pred, gt, 19, 'trainid', crowd)
        assert want[:, 2].sum() + excused == 3000 and (excused > 0) == crowd
        acc, per = run(pred, gt, crowd=crowd, gdt=torch.int64)
        assert_acc(per, want_per)
        assert_acc(acc, want)


def test_image_table_overflow_is_an_error_return(scenes):
    """More distinct pairs than the image's table has slots: result() raises, acc keeps what it held, and after reset() the same
    object is exact again.  An error return of the library: every probe walk is bounded by the table size."""
    from panoptic_forecasting_amd import lib, pq
    preds, gts, ref = scenes
    slots = lib.load().pf_pq_table_slots()
    idx = np.arange(128 * 128, dtype=np.int64).reshape(1, 128, 128)
    pred, gt = idx % (slots + slots // 8) + 11000, idx // 4096
    assert len(np.unique(gt.ravel() * 65536 + pred.ravel())) > slots and pred.max() < 65536
    m = pq.PanopticQuality()
    m.update(dev(preds[:4]), dev(gts[:4]))
    m.result()
    before = m.acc.clone()
    per = torch.full((1, 19, 4), -7.0, dtype=torch.float64, device='cuda')
    m.update(dev(pred), dev(gt), per_image=per)
    with pytest.raises(lib.PfError, match='PF_PQ_STATUS_FULL'):
        m.result()
    assert torch.equal(m.acc, before) and float(per.abs().max()) == 0.0
    m.reset()
    m.update(dev(preds), dev(gts))
    m.result()
    assert_acc(m.acc.cpu().numpy(), ref[0])


@pytest.mark.parametrize('bad,dtype', [(-1, 'i32'), (-1, 'i64'), (65536, 'i32'), (65536, 'i64'), (2 ** 33 + 5, 'i64')])
@pytest.mark.parametrize('which', ['pred', 'gt'])
def test_values_out_of_range_raise(scenes, bad, dtype, which):
    """The flagged image adds nothing, its neighbours in the batch still count."""
    from panoptic_forecasting_amd import lib, pq
    preds, gts, ref = scenes
    p, g = dev(preds[:3], DTYPES[dtype]), dev(gts[:3], DTYPES[dtype])
    (p if which == 'pred' else g)[1, 63, 127] = bad
    m = pq.PanopticQuality()
    per = torch.empty((3, 19, 4), dtype=torch.float64, device='cuda')
    m.update(p, g, per_image=per)
    with pytest.raises(lib.PfError, match='PF_PQ_STATUS_VALUE'):
        m.result()
    want_per = ref[1][:3].copy()
    want_per[1] = 0
    assert_acc(per.cpu().numpy(), want_per)
    assert_acc(m.acc.cpu().numpy(), R.accumulate(preds[[0, 2]], gts[[0, 2]])[0])
    assert m.reset().status() == 0


def test_empty_batch_and_host_tensors():
    from panoptic_forecasting_amd import lib, pq
    m = pq.PanopticQuality()
    m.update(torch.zeros(0, 8, 8, dtype=torch.int32, device='cuda'), torch.zeros(0, 8, 8, dtype=torch.int32, device='cuda'))
    assert m._ws is None and float(m.acc.abs().sum()) == 0.0
    acc = torch.zeros(19, 4, dtype=torch.float64, device='cuda')
    ws = torch.zeros(256, dtype=torch.uint8, device='cuda')
    assert lib.load().pf_pq_accumulate(None, 0, None, 0, 0, 1, 19, 0, 8, 8, acc.data_ptr(), None, ws.data_ptr(), 256, lib.stream_ptr()) == 0
    need = ctypes.c_size_t()
    assert lib.load().pf_pq_workspace(2, ctypes.byref(need)) == 0
    assert lib.load().pf_pq_accumulate(acc.data_ptr(), 0, acc.data_ptr(), 0, 0, 1, 19, 2, 8, 8, acc.data_ptr(), None, ws.data_ptr(), 256,
                                       lib.stream_ptr()) == -2                     # PF_EWORKSPACE
    with pytest.raises(lib.PfError, match='must live on the GPU'):
        m.update(torch.zeros(1, 8, 8, dtype=torch.int32), torch.zeros(1, 8, 8, dtype=torch.int32))
    with pytest.raises(lib.PfError):
        m.update(torch.zeros(1, 3, 5, dtype=torch.int32, device='cuda'), torch.zeros(1, 3, 5, dtype=torch.int32, device='cuda'))


def test_update_does_not_synchronise(scenes):
    from panoptic_forecasting_amd import pq
    preds, gts, ref = scenes
    p, g = dev(preds[:8], torch.int32), dev(gts[:8], torch.int32)
    m = pq.PanopticQuality()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        m.update(p, g)           # first call: allocates the workspace too
        m.update(p, g)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    m.result()
    want = R.accumulate(preds[:8], gts[:8])[0]
    assert np.array_equal(m.acc.cpu().numpy()[:, 1:], 2 * want[:, 1:])


def test_graph_replays_equal_eager(scenes):
    """One captured call on a single stream, replayed five times: the call zeroes its tables itself with kernel nodes, so the
    accumulators are those of five eager calls - counts five-fold, sum_iou the eager value added five times in order."""
    from panoptic_forecasting_amd import pq
    preds, gts, _ = scenes
    p, g = dev(preds[:8], torch.int32), dev(gts[:8], torch.int64)
    eager = pq.PanopticQuality()
    for _ in range(5):
        eager.update(p, g)
    once = pq.PanopticQuality().update(p, g)
    once.result()
    m = pq.PanopticQuality()
    m.update(p, g)               # sizes the workspace outside the capture
    m.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.update(p, g)
    m.reset()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    m.result(), eager.result()
    assert torch.equal(m.acc, eager.acc)
    assert torch.equal(m.acc[:, 1:], 5 * once.acc[:, 1:]) and float(once.acc[:, 1].sum()) > 0


def test_driver_device_matcher_gives_the_host_numbers(tmp_path):
    from panoptic_forecasting_amd import eval_panoptic
    preds, gts = S.make_scenes(n=6, h=64, w=128, seed=7)
    flags = S.write_tree(str(tmp_path), preds, gts)
    host, device = str(tmp_path / 'host.json'), str(tmp_path / 'device.json')
    eval_panoptic.run(eval_panoptic.parse_args(flags + ['--results_file', host, '--matcher', 'host']))
    e = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'panoptic-forecasting_amd', 'eval_panoptic.py')] + flags +
                       ['--results_file', device, '--batch_size', '4', '--num_workers', '2'], capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(host) as f:
        a = json.load(f)
    with open(device) as f:
        b = json.load(f)
    want = R.splits(R.accumulate(R.to_cityscapes(preds), R.to_cityscapes(gts), 19, 'cityscapes', True)[0], scale=1.0)
    for k in ('All', 'Things', 'Stuff'):
        assert a[k]['n'] == b[k]['n'] == want[k]['n'] > 0
        for q in ('pq', 'sq', 'rq'):
            assert abs(a[k][q] - b[k][q]) <= 1e-12 and abs(b[k][q] - want[k][q]) <= 1e-12
    for name in a['per_class']:
        for q in ('pq', 'sq', 'rq'):
            assert abs(a['per_class'][name][q] - b['per_class'][name][q]) <= 1e-12


@pytest.mark.parametrize('matcher', ['device', 'host'])
def test_gather_runs_on_the_device_under_nccl(monkeypatch, tmp_path, matcher):
    """RCCL ("nccl") carries device tensors only: under it the driver must hand gather_accumulators a device tensor for either
    matcher.  Two RCCL ranks cannot share the one GPU of a test machine, so the group is stood in for: is_dist, the backend name
    and the gather itself (which records where its input lives and answers as two equal ranks)."""
    from panoptic_forecasting_amd import dist as pfdist
    from panoptic_forecasting_amd import eval_panoptic
    preds, gts = S.make_scenes(n=2, h=64, w=128, seed=7)
    flags = S.write_tree(str(tmp_path), preds, gts)
    seen = []
    monkeypatch.setattr(pfdist, 'is_dist', lambda: True)
    monkeypatch.setattr(torch.distributed, 'get_backend', lambda: 'nccl')
    monkeypatch.setattr(torch.distributed, 'get_rank', lambda: 0)
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda: 1)
    monkeypatch.setattr(pfdist, 'gather_accumulators', lambda a: seen.append(a.device.type) or torch.stack([a, a]))
    res = eval_panoptic.run(eval_panoptic.parse_args(flags + ['--results_file', str(tmp_path / 'r.json'), '--matcher', matcher]))
    assert seen == ['cuda']
    want = R.splits(2 * R.accumulate(R.to_cityscapes(preds), R.to_cityscapes(gts), 19, 'cityscapes', True)[0], scale=1.0)
    for k in ('All', 'Things', 'Stuff'):
        assert res[k]['n'] == want[k]['n'] and abs(res[k]['pq'] - want[k]['pq']) <= 1e-12


def test_driver_two_gloo_ranks_device_matcher(tmp_path):
    """Two ranks sharing the GPU over gloo, device matcher: the single-process file."""
    import torch.multiprocessing as mp
    import socket
    import pq_eval_worker
    from panoptic_forecasting_amd import eval_panoptic
    preds, gts = S.make_scenes(n=6, h=64, w=128, seed=7)
    flags = S.write_tree(str(tmp_path), preds, gts)
    one, two = str(tmp_path / 'one.json'), str(tmp_path / 'two.json')
    eval_panoptic.run(eval_panoptic.parse_args(flags + ['--results_file', one]))
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(pq_eval_worker.worker, args=(2, port, flags + ['--results_file', two, '--batch_size', '2']), nprocs=2, join=True)
    with open(one) as f:
        a = json.load(f)
    with open(two) as f:
        b = json.load(f)
    for k in ('All', 'Things', 'Stuff'):
        assert a[k]['n'] == b[k]['n'] > 0
        for q in ('pq', 'sq', 'rq'):
            assert abs(a[k][q] - b[k][q]) <= 1e-12


def test_workspace_may_not_grow_around_a_capture_and_float_maps_are_refused(scenes):
    from panoptic_forecasting_amd import lib, pq
    preds, gts, _ = scenes
    p, g = dev(preds[:8], torch.int32), dev(gts[:8], torch.int32)
    with pytest.raises(lib.PfError, match='integer label map'):
        pq.PanopticQuality().update(p.float(), g)
    with pytest.raises(lib.PfError, match='integer label map'):
        pq.PanopticQuality().update(p, g.bool())
    small = pq.PanopticQuality().update(dev(preds[:4], torch.int16), dev(gts[:4], torch.int16))
    small.result()
    assert_acc(small.acc.cpu().numpy(), R.accumulate(preds[:4], gts[:4])[0])      # i16 maps are widened, not refused
    m = pq.PanopticQuality()
    m.update(p[:2], g[:2])
    m.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.update(p[:2], g[:2])
    graph.replay()
    torch.cuda.synchronize()
    with pytest.raises(lib.PfError, match='after a graph capture'):
        m.update(p, g)                                                             # B = 8 would replace the captured workspace
    m.update(p[:1], g[:1])                                                         # a smaller batch still fits
    m.result()
