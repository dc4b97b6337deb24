"""Semantic IoU on the device: pf_confusion_accumulate / semantic_iou.SemanticIoU (csrc/confusion_kernels.hip) against
tests/conf_ref64.py.  The tables are integers: every comparison is equality, per_image included."""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import conf_ref64 as C
import conf_scenes as CS

pytestmark = pytest.mark.gpu
KINDS = {'u8': torch.uint8, 'i32': torch.int32, 'i64': torch.int64}
FMTS = ('trainid', 'cityscapes')
CHUNK = 16384                                  # pf_confusion_chunk_pixels(): checked below, the shapes are written out from it
_REF = {}


def checkerboard(h=1024, w=2048):
    odd = (np.add.outer(np.arange(h), np.arange(w)) % 2).astype(bool)[None]
    return np.where(odd, 3, 8).astype(np.int64), np.where(odd, 3, 5).astype(np.int64)


SHAPES = {
    'smallest': lambda: CS.run_maps((1, 1, 1), 1),
    'all head and tail': lambda: CS.run_maps((2, 3, 5), 2),
    'odd width': lambda: CS.run_maps((1, 7, 33), 3),
    'exact trips': lambda: CS.run_maps((3, 16, 64), 4),
    'chunk - 1': lambda: CS.run_maps((2, 127, 129), 5),
    'chunk': lambda: CS.run_maps((2, 128, 128), 6),
    'chunk + 1': lambda: CS.run_maps((2, 5, 3277), 7),
    'several chunks': lambda: CS.run_maps((2, 200, 333), 8),
    'constant 1024x2048': lambda: (np.full((1, 1024, 2048), 7, np.int64), np.full((1, 1024, 2048), 7, np.int64)),
    'checkerboard 1024x2048': checkerboard,
}


def reference(name, fmt, n_cls=19):
    """(pred, gt, table, per_image) of a named case in ``fmt``: computed once, shared, read-only."""
    key = (name, fmt, n_cls)
    if key not in _REF:
        pred, gt = SHAPES[name]()
        if fmt == 'cityscapes':
            pred, gt = C.to_cityscapes(pred), C.to_cityscapes(gt)
        table, per = C.confusion(pred, gt, n_cls, fmt)
        for a in (pred, gt, table, per):
            a.setflags(write=False)
        _REF[key] = (pred, gt, table, per)
    return _REF[key]


def dev(a, dtype=torch.uint8):
    return torch.from_numpy(np.array(a)).to('cuda', dtype)


def run(pred, gt, fmt='trainid', n_cls=19):
    """pred, gt: device tensors -> (acc, per_image) numpy, after result() found a clean status word."""
    from panoptic_forecasting_amd import semantic_iou as si
    m = si.SemanticIoU(n_cls, fmt)
    per = torch.full((len(pred), 20, 20), -7, dtype=torch.int64, device='cuda')
    m.update(pred, gt, per_image=per)
    m.result()
    return m.acc.cpu().numpy(), per.cpu().numpy()


def test_the_chunk_constant_is_the_one_the_shapes_were_written_for():
    from panoptic_forecasting_amd import lib
    assert lib.load().pf_confusion_chunk_pixels() == CHUNK
    assert 127 * 129 == CHUNK - 1 and 128 * 128 == CHUNK and 5 * 3277 == CHUNK + 1 and 200 * 333 > 4 * CHUNK


@pytest.mark.parametrize('name', list(SHAPES))
def test_tables_equal_the_restatement_for_every_kind_pair_and_format(name):
    for fmt in FMTS:
        pred, gt, want, want_per = reference(name, fmt)
        assert want.sum() == pred.size
        maps = {k: (dev(pred, dt), dev(gt, dt)) for k, dt in KINDS.items()}
        for pk in KINDS:
            for gk in KINDS:
                acc, per = run(maps[pk][0], maps[gk][1], fmt)
                assert np.array_equal(per, want_per), (fmt, pk, gk, np.argwhere(per != want_per)[:8].tolist())
                assert np.array_equal(acc, want), (fmt, pk, gk)


@pytest.mark.parametrize('fmt', FMTS)
def test_misaligned_base_pointers(fmt):
    """[1:] of a flat parent of 1 + 2*64*100 elements: the base is one element past an aligned address - 1 byte for u8, 4 for i32,
    8 for i64; H*W = 6400 keeps image 1 as far off as image 0.  Both maps shifted: a head of 15 (u8 x u8) or 3 pixels aligns both.
    Only the prediction shifted: no head aligns both, and the ground truth is read by element loads."""
    pred, gt = CS.run_maps((2, 64, 100), 9)
    if fmt == 'cityscapes':
        pred, gt = C.to_cityscapes(pred), C.to_cityscapes(gt)
    want, want_per = C.confusion(pred, gt, 19, fmt)

    def shifted(a, dt):
        parent = torch.zeros(1 + a.size, dtype=dt, device='cuda')
        parent[1:] = dev(a.ravel(), dt)
        view = parent[1:].view(a.shape)
        assert view.is_contiguous() and view.data_ptr() % 16 == parent.element_size()
        return view

    for pk, pdt in KINDS.items():
        for gk, gdt in KINDS.items():
            for g in (shifted(gt, gdt), dev(gt, gdt)):
                acc, per = run(shifted(pred, pdt), g, fmt)
                assert np.array_equal(per, want_per) and np.array_equal(acc, want), (pk, gk, g.data_ptr() % 16)


def test_runs_do_not_leak_between_images():
    """The last pixel of image 0 and the first of image 1 share a pair, which image 1 holds nowhere else."""
    for shape in ((2, 4, 16), (2, 3, 5), (2, 128, 128)):
        pred, gt = np.full(shape, 2, np.int64), np.full(shape, 4, np.int64)
        pred[0, -1, -1], gt[0, -1, -1] = 9, 9
        pred[1, 0, 0], gt[1, 0, 0] = 9, 9
        n = shape[1] * shape[2]
        want_per = np.zeros((2, 20, 20), np.int64)
        want_per[:, 4, 2], want_per[:, 9, 9] = n - 1, 1
        assert np.array_equal(C.confusion(pred, gt)[1], want_per)
        for k, dt in KINDS.items():
            acc, per = run(dev(pred, dt), dev(gt, dt))
            assert np.array_equal(per, want_per) and np.array_equal(acc, want_per.sum(0)), (shape, k)


def test_acc_is_added_to_and_n_cls_sends_the_rest_to_void():
    from panoptic_forecasting_amd import semantic_iou as si
    pred, gt = CS.make_scenes(n=4)
    m = si.SemanticIoU()
    m.update(dev(pred[:3]), dev(gt[:3]))
    m.update(dev(pred[3:], torch.int64), dev(gt[3:], torch.int32))
    assert m.result()['All']['n'] > 0
    assert np.array_equal(m.acc.cpu().numpy(), C.confusion(pred, gt)[0])
    want = C.iou(C.confusion(pred, gt)[0])
    assert all(m.result()[k]['n'] == want[k]['n'] and abs(m.result()[k]['miou'] - want[k]['miou']) <= 1e-12 * want[k]['miou']
               for k in ('All', 'Stuff', 'MO'))
    for fmt in FMTS:
        p, g = (pred, gt) if fmt == 'trainid' else (C.to_cityscapes(pred), C.to_cityscapes(gt))
        want, want_per = C.confusion(p, g, 11, fmt)
        assert want[11:19].sum() == 0 and want[:, 11:19].sum() == 0 and want[19].sum() > C.confusion(p, g, 19, fmt)[0][19].sum()
        acc, per = run(dev(p), dev(g), fmt, n_cls=11)
        assert np.array_equal(per, want_per) and np.array_equal(acc, want)


@pytest.mark.parametrize('bad,kind', [(256, 'i32'), (-1, 'i32'), (256, 'i64'), (-1, 'i64'), (2 ** 33 + 5, 'i64')])
@pytest.mark.parametrize('which', ['pred', 'gt'])
def test_values_out_of_range_set_the_flag(bad, kind, which):
    """The flagged image adds nothing and its block is zero, its neighbours still count; result() raises, reset() clears."""
    from panoptic_forecasting_amd import lib, semantic_iou as si
    pred, gt = CS.make_scenes(n=3)
    want_per = C.confusion(pred, gt)[1].copy()
    want_per[1] = 0
    for at in ((1, 63, 127), (1, 0, 0), (1, 20, 77)):            # the last pixel, the first, mid-image
        p, g = dev(pred, KINDS[kind]), dev(gt, KINDS[kind])
        (p if which == 'pred' else g)[at] = bad
        m = si.SemanticIoU()
        per = torch.full((3, 20, 20), -7, dtype=torch.int64, device='cuda')
        m.update(p, g, per_image=per)
        with pytest.raises(lib.PfError, match='PF_CONF_STATUS_VALUE'):
            m.result()
        assert m.status() == 1
        assert np.array_equal(per.cpu().numpy(), want_per) and np.array_equal(m.acc.cpu().numpy(), want_per.sum(0))
        assert m.reset().status() == 0 and int(m.acc.abs().sum()) == 0
        m.update(dev(pred), dev(gt))
        m.result()
        assert np.array_equal(m.acc.cpu().numpy(), C.confusion(pred, gt)[0])
    odd_p, odd_g = dev(pred[:1, :3, :5], KINDS[kind]).contiguous(), dev(gt[:1, :3, :5], KINDS[kind]).contiguous()   # head / tail lanes only
    (odd_p if which == 'pred' else odd_g)[0, 2, 4] = bad
    m = si.SemanticIoU().update(odd_p, odd_g)
    assert m.status() == 1 and int(m.acc.abs().sum()) == 0


def test_empty_batch_wrong_dtypes_shapes_and_host_tensors():
    from panoptic_forecasting_amd import lib, semantic_iou as si
    m = si.SemanticIoU()
    z = lambda *s, dt=torch.uint8, d='cuda': torch.zeros(*s, dtype=dt, device=d)
    m.update(z(0, 8, 8), z(0, 8, 8))
    assert m._ws is None and int(m.acc.abs().sum()) == 0 and m.status() == 0
    L = lib.load()
    ws = z(256)
    assert L.pf_confusion_accumulate(None, 0, None, 0, 0, 19, 0, 8, 8, m.acc.data_ptr(), None, ws.data_ptr(), 256, lib.stream_ptr()) == 0
    need = ctypes.c_size_t()
    assert L.pf_confusion_workspace(2, ctypes.byref(need)) == 0 and need.value >= 256 + 2 * 1600
    a = m.acc.data_ptr()
    assert L.pf_confusion_accumulate(a, 0, a, 0, 0, 19, 2, 8, 8, a, None, ws.data_ptr(), 256, lib.stream_ptr()) == -2      # PF_EWORKSPACE
    assert L.pf_confusion_accumulate(a, 3, a, 0, 0, 19, 2, 8, 8, a, None, ws.data_ptr(), 256, lib.stream_ptr()) == -1      # PF_EINVAL
    assert L.pf_confusion_accumulate(a, 0, a, 0, 0, 20, 2, 8, 8, a, None, ws.data_ptr(), 256, lib.stream_ptr()) == -1
    assert L.pf_confusion_accumulate(a + 4, 2, a, 0, 0, 19, 2, 8, 8, a, None, ws.data_ptr(), 256, lib.stream_ptr()) == -1  # i64 at +4
    torch.cuda.synchronize()
    assert int(m.acc.abs().sum()) == 0
    with pytest.raises(lib.PfError, match='must live on the GPU'):
        m.update(z(1, 8, 8, d='cpu'), z(1, 8, 8, d='cpu'))
    with pytest.raises(lib.PfError, match='must live on the GPU'):
        m.update(z(1, 8, 8), z(1, 8, 8, d='cpu'))
    with pytest.raises(lib.PfError, match='integer label map'):
        m.update(z(1, 8, 8, dt=torch.float32), z(1, 8, 8))
    with pytest.raises(lib.PfError, match='integer label map'):
        m.update(z(1, 8, 8), z(1, 8, 8, dt=torch.bool))
    with pytest.raises(lib.PfError, match='one shape'):
        m.update(z(1, 8, 8), z(1, 8, 9))
    with pytest.raises(lib.PfError, match='one shape'):
        m.update(z(8, 8), z(8, 8))
    with pytest.raises(lib.PfError, match='contiguous'):
        m.update(z(1, 8, 16)[:, :, ::2], z(1, 8, 8))
    with pytest.raises(lib.PfError, match='per_image'):
        m.update(z(1, 8, 8), z(1, 8, 8), per_image=z(1, 19, 19, dt=torch.int64))
    with pytest.raises(lib.PfError, match='per_image'):
        m.update(z(1, 8, 8), z(1, 8, 8), per_image=z(1, 20, 20, dt=torch.float64))
    with pytest.raises(lib.PfError, match='runs on the GPU'):
        si.SemanticIoU(device='cpu')
    pred, gt = CS.make_scenes(n=2)
    small = si.SemanticIoU().update(dev(pred, torch.int16), dev(gt, torch.int16))            # i16 maps are widened, not refused
    small.result()
    assert np.array_equal(small.acc.cpu().numpy(), C.confusion(pred, gt)[0])


def test_two_runs_give_equal_bits_and_update_does_not_synchronise():
    from panoptic_forecasting_amd import semantic_iou as si
    pred, gt = CS.make_scenes(n=8)
    p, g = dev(pred), dev(gt)
    one, two = si.SemanticIoU(), si.SemanticIoU()
    pa, pb = torch.empty(8, 20, 20, dtype=torch.int64, device='cuda'), torch.empty(8, 20, 20, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        one.update(p, g, per_image=pa)           # first call: allocates the workspace too
        two.update(p, g, per_image=pb)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    one.result(), two.result()
    assert torch.equal(one.acc, two.acc) and torch.equal(pa, pb)
    assert np.array_equal(one.acc.cpu().numpy(), C.confusion(pred, gt)[0])


def test_graph_replays_equal_eager_and_the_workspace_may_not_grow_around_a_capture(monkeypatch):
    """One update captured on torch.cuda.graph's side stream after a warm-up update at that B, replayed five times with acc
    re-zeroed in between: every replay gives the eager table (the call zeroes its tables itself, with kernel nodes)."""
    from panoptic_forecasting_amd import lib, semantic_iou as si
    pred, gt = CS.make_scenes(n=4)
    p, g = dev(pred), dev(gt, torch.int32)
    eager = si.SemanticIoU().update(p, g)
    eager.result()
    assert int(eager.acc.sum()) == pred.size
    m = si.SemanticIoU()
    per = torch.zeros(4, 20, 20, dtype=torch.int64, device='cuda')
    m.update(p, g, per_image=per)               # sizes the workspace outside the capture
    m.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.update(p, g, per_image=per)
    for rep in range(5):
        m.acc.zero_()
        per.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(m.acc, eager.acc), rep
        assert torch.equal(per.sum(0), eager.acc), rep
    m.result()
    big_p, big_g = dev(np.concatenate([pred, pred])), dev(np.concatenate([gt, gt]))
    with pytest.raises(lib.PfError, match='after a graph capture'):
        m.update(big_p, big_g)                   # B = 8 would replace the captured workspace
    m.update(p[:1], g[:1])                       # a smaller batch still fits
    m.result()
    fresh = si.SemanticIoU().update(p[:1], g[:1])
    fresh.result()
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)   # no capture is begun only to be abandoned
    with pytest.raises(lib.PfError, match='during a graph capture'):
        fresh.update(p, g)


def _clean_env():
    return {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}


@pytest.mark.parametrize('fmt', FMTS)
def test_driver_device_matcher_gives_the_host_file(tmp_path, fmt):
    from panoptic_forecasting_amd import eval_semantic
    pred, gt = CS.make_scenes(n=3, h=32, w=48, seed=9)
    flags = CS.write_tree(str(tmp_path), pred, gt, fmt)
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
    assert a == b and a['All']['n'] > 0                      # the same integers through the same formula: the same file
    assert np.array_equal(np.array(b['confusion']), C.confusion(pred, gt)[0])


def test_driver_two_gloo_ranks_equal_the_single_process_file(tmp_path):
    """Two ranks sharing the GPU over gloo, device matcher: integer tables add exactly, so the file is the single process's."""
    import torch.multiprocessing as mp
    import conf_eval_worker
    from panoptic_forecasting_amd import eval_semantic
    pred, gt = CS.make_scenes(n=5, h=32, w=48, seed=9)
    flags = CS.write_tree(str(tmp_path), pred, gt, 'cityscapes')
    one, two = str(tmp_path / 'one.json'), str(tmp_path / 'two.json')
    eval_semantic.run(eval_semantic.parse_args(flags + ['--results_file', one]))
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(conf_eval_worker.worker, args=(2, port, flags + ['--results_file', two, '--batch_size', '2']), nprocs=2, join=True)
    with open(one) as f:
        a = json.load(f)
    with open(two) as f:
        b = json.load(f)
    assert a == b and a['All']['n'] > 0


def test_export_semantic_end_to_end(tmp_path):
    """odometry / bg export files on disk -> export_semantic.main -> one PNG per scene, whose content is predict_semantics of the
    same batch converted trainId -> id; the frame without a prediction is filled in; eval_semantic reads the tree."""
    import yaml
    import fg_ref64 as R
    import fgscene_tree as FT
    from panoptic_forecasting_amd import eval_semantic, export_semantic, fg_dataset as D, hop_io
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

    out = export_semantic.main(['--config_file', str(ckpt_dir / 'config.yaml'), '--load_model', str(ckpt_dir / 'fg_model.pt'),
                                '--export_name', 'sem', '--working_dir', str(tmp_path / 'work')])
    result_dir, written, missing = out[FT.SPLIT]
    assert result_dir == os.path.join(str(tmp_path / 'work'), 'sem_val') and missing == 1
    names = ['synth_%s_000019_gtFine_labelIds.png' % seq for seq in ('000001', '000002')]
    assert [os.path.relpath(p, result_dir) for p in written] == [os.path.join('synth', n) for n in names]
    assert sorted(os.listdir(os.path.join(result_dir, 'synth'))) == names + ['synth_000009_000019_gtFine_labelIds.png']

    ds = D.NativeFGSceneDataset(FT.SPLIT, {'data': dict(data)}, test=True)
    host = ds.host_batch(range(2))
    with torch.no_grad():
        seg = model.predict_semantics(host['inputs'], host['labels'])['seg']
    assert seg.dtype == torch.int64 and ((seg >= 11) & (seg < 19)).any() and (seg < 11).any() and int(seg.max()) <= 255
    for b in range(2):
        got = hop_io.read_png(written[b])
        assert got.shape == (1024, 2048) and got.dtype == np.uint8
        assert np.array_equal(got, C.to_cityscapes(seg[b].cpu().numpy())), b
    res = eval_semantic.run(eval_semantic.parse_args(['--gt-folder', result_dir, '--prediction-folder', result_dir,
                                                      '--results_file', str(tmp_path / 'miou.json'), '--batch_size', '2']))
    assert res['All']['n'] > 0 and res['All']['miou'] == 1.0 and res['MO']['n'] > 0 and res['pixel_acc'] == 1.0
