"""pf_bg_augment (csrc/bg_augment.hip) and the native bg loader on the device: against fixture G12 (the reference's transforms),
against the numpy statement of the gather, against pf_hop_load, under capture, and through train_bg.py --dataset native."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
LO, HI = 0.1, 200.0


def dev(a):
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(seg, label, depth, tabs, **kw):
    """numpy sources [B,T,H,W] / [B,H,W] / [B,T,H,W] u16 and four [B,n] tables -> the kernel's four outputs as numpy."""
    from panoptic_forecasting_amd import bg_augment as A
    t = [dev(np.asarray(x, np.int32)) for x in tabs]
    out = A.device_augment(dev(seg), dev(label) if label is not None else None, dev(depth) if depth is not None else None,
                           t[0], t[1], t[2], t[3], LO, HI, **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() if o is not None else None for o in out]


def want(seg, label, depth, tabs, pad=255):
    """The numpy gather + oracle.hop's decode: (seg, label, depth f32, mask bool)."""
    from oracle import hop as oh
    from panoptic_forecasting_amd import bg_augment as A
    y_map, x_map, y_arr, x_arr = tabs
    b = seg.shape[0]
    o_seg = np.stack([A.gather_numpy(seg[i], y_map[i], x_map[i], pad) for i in range(b)])
    o_lab = np.stack([A.gather_numpy(label[i], y_map[i], x_map[i], pad) for i in range(b)]) if label is not None else None
    o_dep = o_msk = None
    if depth is not None:
        codes = np.stack([A.gather_numpy(depth[i], y_arr[i], x_arr[i], 0) for i in range(b)])
        d, m = oh.load_depth(codes, LO, HI)
        o_dep, o_msk = d.numpy(), m.numpy()
    return o_seg, o_lab, o_dep, o_msk


def assert_same(got, exp):
    for g, e, name in zip(got, exp, ('seg', 'label', 'depth', 'mask')):
        if e is None:
            assert g is None, name
        elif name == 'depth':
            assert np.array_equal(g.view(np.int32), e.view(np.int32)), name      # f32 bits
        else:
            assert g.dtype == e.dtype and np.array_equal(g, e), name


def random_sources(g, b, t, h, w):
    seg = g.randint(0, 20, (b, t, h, w)).astype(np.uint8)
    label = g.randint(0, 20, (b, h, w)).astype(np.uint8)
    depth = g.randint(0, 65536, (b, t, h, w)).astype(np.uint16)
    depth[g.rand(b, t, h, w) < 0.2] = 0
    depth[:, :, 0, :5] = [0, 255, 256, 257, 65535]
    return seg, label, depth


def test_kernel_equals_the_reference_transforms_bit_for_bit():
    """Every case of G12 (sources of two sizes -> one launch each group): seg, label and mask equal the reference's planes, depth
    equals oracle.hop's decode of the reference's u16 planes in f32 bits."""
    from oracle import hop as oh
    from panoptic_forecasting_amd import bg_augment as A
    z = np.load(os.path.join(G, 'g12_bgaug.npz'))
    cases = [{k[len('c%d_' % i):]: z[k] for k in z.files if k.startswith('c%d_' % i)} for i in range(int(z['n_cases']))]
    for shape in sorted({c['src_label'].shape for c in cases}):
        group = [c for c in cases if c['src_label'].shape == shape]
        h, w = shape
        tabs = [[], [], [], []]
        for c in group:
            p = A.draw_params(random.Random(int(c['seed'])), w, h, int(c['size']), float(c['scale_min']), float(c['scale_max']))
            for dst, tab in zip(tabs, A.build_tables(p, w, h, int(c['size']))):
                dst.append(tab)
        got = run(np.stack([c['src_seg'] for c in group]), np.stack([c['src_label'] for c in group]),
                  np.stack([c['src_depth'] for c in group]), [np.stack(t) for t in tabs])
        d, m = oh.load_depth(np.stack([c['out_depth'] for c in group]), LO, HI)
        assert_same(got, (np.stack([c['out_seg'] for c in group]), np.stack([c['out_label'] for c in group]), d.numpy(), m.numpy()))
        assert len(group) >= 6


@pytest.mark.parametrize('t', [1, 3])
@pytest.mark.parametrize('ow', [40, 37])
def test_random_tables_and_padding_entries(t, ow):
    """B = 3, oh = 21 (three row blocks, the last ragged), ow = 40 (16-B / 4-B stores) and 37 (scalar stores, ragged last quad);
    entries -1, -5, Ws / Hs and 2^30 are padding and are not followed."""
    g = np.random.RandomState(100 * t + ow)
    b, h, w, oh = 3, 19, 53, 21
    seg, label, depth = random_sources(g, b, t, h, w)
    tabs = [g.randint(0, h, (b, oh)), g.randint(0, w, (b, ow)), g.randint(0, h, (b, oh)), g.randint(0, w, (b, ow))]
    for tab, extent in zip(tabs, (h, w, h, w)):
        n = tab.shape[1]
        for i, bad in enumerate((-1, -5, extent, 2 ** 30)):
            tab[i % b, g.randint(0, n)] = bad
        tab[2, n - 1] = extent              # the last column / row too
    tabs = [x.astype(np.int32) for x in tabs]
    assert_same(run(seg, label, depth, tabs), want(seg, label, depth, tabs))
    got = run(seg, label, depth, tabs, pad_label=7)
    assert_same(got[:2], want(seg, label, depth, tabs, pad=7)[:2])


def test_identity_tables_equal_hop_load():
    from panoptic_forecasting_amd import bg_augment as A
    from panoptic_forecasting_amd import hop_io
    g = np.random.RandomState(5)
    b, t, h, w = 2, 3, 24, 44
    seg, label, depth = random_sources(g, b, t, h, w)
    tab = A.build_tables(None, w, h, None)
    tabs = [np.stack([x] * b) for x in tab]
    got = run(seg, label, depth, tabs)
    d, m = hop_io.device_load_depth(dev(depth), LO, HI)
    assert np.array_equal(got[2].view(np.int32), d.cpu().numpy().view(np.int32)) and np.array_equal(got[3], m.cpu().numpy())
    assert np.array_equal(got[0], seg) and np.array_equal(got[1], label)


def test_full_size_batch():
    """B = 2, 1024 x 2048 -> 800 x 800 with drawn parameters (one of them flipped and padded in h)."""
    from panoptic_forecasting_amd import bg_augment as A
    g = np.random.RandomState(9)
    b, t, h, w, size = 2, 3, 1024, 2048, 800
    seg, label, depth = random_sources(g, b, t, h, w)
    ps = [{'crop_w': 1100, 'crop_h': 1100, 'pad_w': 0, 'pad_h': 39, 'x1': 948, 'y1': 2, 'flip': True},
          A.draw_params(random.Random(4), w, h, size, 0.5, 2.0)]
    tabs = [np.stack(x) for x in zip(*[A.build_tables(p, w, h, size) for p in ps])]
    assert (tabs[0][0] < 0).any() and tabs[1][0][0] > tabs[1][0][-1]
    assert_same(run(seg, label, depth, tabs), want(seg, label, depth, tabs))


def test_nullable_label_and_depth_and_empty_batch():
    from panoptic_forecasting_amd import bg_augment as A
    g = np.random.RandomState(11)
    b, t, h, w, oh, ow = 2, 3, 17, 29, 12, 20
    seg, label, depth = random_sources(g, b, t, h, w)
    tabs = [g.randint(-2, h + 2, (b, oh)).astype(np.int32), g.randint(-2, w + 2, (b, ow)).astype(np.int32),
            g.randint(-2, h + 2, (b, oh)).astype(np.int32), g.randint(-2, w + 2, (b, ow)).astype(np.int32)]
    assert_same(run(seg, None, depth, tabs), want(seg, None, depth, tabs))
    assert_same(run(seg, label, None, tabs), want(seg, label, None, tabs))
    assert_same(run(seg, None, None, tabs), want(seg, None, None, tabs))
    # outputs of an absent input are not written
    out = (torch.full((b, t, oh, ow), 9, dtype=torch.uint8, device='cuda'), torch.full((b, oh, ow), 9, dtype=torch.uint8, device='cuda'),
           torch.full((b, t, oh, ow), 9.0, device='cuda'), torch.full((b, t, oh, ow), 9, dtype=torch.uint8, device='cuda'))
    A.device_augment(dev(seg), None, None, dev(tabs[0]), dev(tabs[1]), None, None, LO, HI, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), want(seg, None, None, tabs)[0])
    assert all(bool((o == 9).all()) for o in out[1:])
    # B = 0 launches nothing and succeeds
    e = lambda *s: torch.empty(s, dtype=torch.uint8, device='cuda')      # noqa: E731
    i = lambda *s: torch.empty(s, dtype=torch.int32, device='cuda')      # noqa: E731
    o = A.device_augment(e(0, t, h, w), e(0, h, w), torch.empty((0, t, h, w), dtype=torch.int16, device='cuda'),
                         i(0, oh), i(0, ow), i(0, oh), i(0, ow), LO, HI)
    torch.cuda.synchronize()
    assert o[0].shape == (0, t, oh, ow) and o[2].shape == (0, t, oh, ow)


def test_unaligned_outputs_take_scalar_stores():
    """ow % 4 == 0 but the output bases off the 16-B / 4-B grid (views one element into larger buffers): the launch falls back to
    scalar stores and writes the same values, and nothing either side of the views."""
    from panoptic_forecasting_amd import bg_augment as A
    g = np.random.RandomState(17)
    b, t, h, w, oh, ow = 2, 3, 19, 31, 13, 24
    seg, label, depth = random_sources(g, b, t, h, w)
    tabs = [g.randint(-1, h + 1, (b, oh)).astype(np.int32), g.randint(-1, w + 1, (b, ow)).astype(np.int32),
            g.randint(-1, h + 1, (b, oh)).astype(np.int32), g.randint(-1, w + 1, (b, ow)).astype(np.int32)]
    n, nl = b * t * oh * ow, b * oh * ow
    bufs = [torch.full((n + 2,), 9, dtype=torch.uint8, device='cuda'), torch.full((nl + 2,), 9, dtype=torch.uint8, device='cuda'),
            torch.full((n + 2,), 9.0, device='cuda'), torch.full((n + 2,), 9, dtype=torch.uint8, device='cuda')]
    out = (bufs[0][1:n + 1].view(b, t, oh, ow), bufs[1][1:nl + 1].view(b, oh, ow), bufs[2][1:n + 1].view(b, t, oh, ow),
           bufs[3][1:n + 1].view(b, t, oh, ow))
    assert out[2].data_ptr() % 16 == 4 and out[0].data_ptr() % 4 == 1
    got = A.device_augment(dev(seg), dev(label), dev(depth), *[dev(x) for x in tabs], LO, HI, out=out)
    torch.cuda.synchronize()
    assert_same([o.cpu().numpy() for o in got], want(seg, label, depth, tabs))
    assert all(float(x[0]) == 9 and float(x[-1]) == 9 for x in bufs)


def test_offsets_past_2_to_the_31():
    """B = 2, T = 2 planes of 32768 x 32768: the last seg plane starts 3 * 2^30 bytes in, the last depth plane 3 * 2^31 bytes in; the
    tables point at the far corner of every plane.  Sources are made and gathered on the device."""
    from oracle import hop as oh_
    from panoptic_forecasting_amd import bg_augment as A
    b, t, s, oh, ow = 2, 2, 32768, 9, 12
    g = torch.Generator(device='cuda').manual_seed(23)
    seg = torch.randint(0, 20, (b, t, s, s), generator=g, dtype=torch.uint8, device='cuda')
    lab = torch.randint(0, 20, (b, s, s), generator=g, dtype=torch.uint8, device='cuda')
    dep = torch.randint(-32768, 32768, (b, t, s, s), generator=g, dtype=torch.int16, device='cuda')
    r = np.random.RandomState(23)
    tabs = [r.randint(s - 64, s, (b, n)).astype(np.int32) for n in (oh, ow, oh, ow)]
    tabs[0][1, 0], tabs[1][0, 3] = s, -1
    td = [dev(x) for x in tabs]
    got = A.device_augment(seg, lab, dep, *td, LO, HI)
    torch.cuda.synchronize()

    def pick(src, yt, xt, pad):       # [.., s, s] on the device -> [.., oh, ow] numpy
        y, x = torch.from_numpy(yt).long().cuda(), torch.from_numpy(xt).long().cuda()
        v = src[..., y.clamp(0, s - 1), :][..., x.clamp(0, s - 1)].clone()
        v[..., (y < 0) | (y >= s), :] = pad
        v[..., (x < 0) | (x >= s)] = pad
        return v.cpu().numpy()
    w_seg = np.stack([pick(seg[i], tabs[0][i], tabs[1][i], 255) for i in range(b)])
    w_lab = np.stack([pick(lab[i], tabs[0][i], tabs[1][i], 255) for i in range(b)])
    codes = np.stack([pick(dep[i], tabs[2][i], tabs[3][i], 0) for i in range(b)]).view(np.uint16)
    d, m = oh_.load_depth(codes, LO, HI)
    assert_same([o.cpu().numpy() for o in got], (w_seg, w_lab, d.numpy(), m.numpy()))


def test_captured_launch_replays():
    from panoptic_forecasting_amd import bg_augment as A
    g = np.random.RandomState(13)
    b, t, h, w, oh, ow = 2, 3, 33, 47, 24, 40
    seg, label, depth = random_sources(g, b, t, h, w)
    tabs = [g.randint(-1, h + 1, (b, oh)).astype(np.int32), g.randint(-1, w + 1, (b, ow)).astype(np.int32),
            g.randint(-1, h + 1, (b, oh)).astype(np.int32), g.randint(-1, w + 1, (b, ow)).astype(np.int32)]
    src = [dev(seg), dev(label), dev(depth)] + [dev(x) for x in tabs]
    eager = [o.clone() for o in A.device_augment(*src, LO, HI)]
    out = (torch.zeros((b, t, oh, ow), dtype=torch.uint8, device='cuda'), torch.zeros((b, oh, ow), dtype=torch.uint8, device='cuda'),
           torch.zeros((b, t, oh, ow), device='cuda'), torch.zeros((b, t, oh, ow), dtype=torch.uint8, device='cuda'))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        A.device_augment(*src, LO, HI, out=out)
    for _ in range(5):
        for o in out:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
        assert torch.equal(out[2].view(torch.int32), eager[2].view(torch.int32)) and torch.equal(out[3].view(torch.bool), eager[3])
    assert_same([o.cpu().numpy() for o in eager], want(seg, label, depth, tabs))


# ---------------------------------------------------------------------------------------------- loader + driver
def make_tree(root, h=64, w=128):
    from PIL import Image
    g = np.random.RandomState(21)
    dirs = [os.path.join(root, 'frame%d' % i) for i in range(3)]
    frames = [('train', 'aachen' if i < 5 else 'ulm', '%06d' % i, 19) for i in range(8)] + [('val', 'bonn', '%06d' % i, 19) for i in range(2)]
    for split, city, seq, frame in frames:
        os.makedirs(os.path.join(root, 'gt', split, city), exist_ok=True)
        coarse = g.randint(0, 12, (h // 8, w // 8)).astype(np.uint8)
        coarse[coarse == 11] = 255
        lab = np.kron(coarse, np.ones((8, 8), np.uint8))
        Image.fromarray(lab).save(os.path.join(root, 'gt', split, city, '%s_%s_%06d_gtFine_labelTrainIds.png' % (city, seq, frame)))
        for d in dirs:
            os.makedirs(os.path.join(d, split, city), exist_ok=True)
            noisy = np.where(g.rand(h, w) < 0.1, g.randint(0, 11, (h, w)), lab).astype(np.uint8)
            Image.fromarray(noisy).save(os.path.join(d, split, city, '%s_%s_%06d_gtFine_labelIds.png' % (city, seq, frame)))
            q = np.where(g.rand(h, w) < 0.2, 0, (g.rand(h, w) * 60 + 1) * 256).astype(np.uint16)
            Image.fromarray(q).save(os.path.join(d, split, city, '%s_%s_%06d_depths.png' % (city, seq, frame)))
    return dirs


def tree_config(root, dirs, path):
    import yaml
    cfg = {'task': 'bg', 'model': {'model_type': 'bg', 'num_inputs': 3, 'use_depth_inps': True, 'convert2onehot': True},
           'data': {'data_dir': dirs, 'gt_dir': os.path.join(root, 'gt'), 'cityscapes_dir': root, 'data_splits': ['train', 'val'],
                    'use_depths': True, 'depth_h5_path': os.path.join(root, 'depth_%s.h5'), 'min_depth': 0.1, 'max_depth': 200,
                    'only_background': True, 'crop_size': 64, 'scale_min': 0.5, 'scale_max': 2.0, 'gap_len': [3],
                    'depth_norm_params': [20.0, 15.0]},
           'training': {'batch_size': 2, 'val_batch_size': 2, 'num_epochs': 2, 'lr': 2.0e-3, 'mom': 0.9, 'wd': 1.0e-4,
                        'clip_grad_norm': 5.0, 'num_data_workers': 1}}
    with open(path, 'w') as f:
        yaml.safe_dump(cfg, f)
    return cfg


def test_loader_batches_equal_the_host_gather(tmp_path):
    """NativeBatches end to end (decode -> pinned -> side-stream upload -> kernel): every batch of an epoch equals the numpy gather of
    the decoded files under the sample's own parameters, with 1 and with 4 threads; validation is the identity."""
    from panoptic_forecasting_amd import bg_augment as A
    from panoptic_forecasting_amd import bg_dataset as D
    from panoptic_forecasting_amd import hop_io
    root = str(tmp_path)
    params = tree_config(root, make_tree(root), os.path.join(root, 'cfg.yaml'))
    params['seed'] = 3
    ds = D.build_dataset(params)
    for threads in (1, 4):
        loader = D.NativeBatches(ds['train'], params, 0, 1, train=True, threads=threads)
        plan = loader.index_batches(2)
        got = list(loader.batches(2))
        loader.close()
        assert len(got) == len(plan) == 4
        for batch, idxs in zip(got, plan):
            segs = np.stack([np.stack([hop_io.read_png(f) for f in ds['train'].samples[i]['data_files']]) for i in idxs])
            labs = np.stack([hop_io.read_png(ds['train'].samples[i]['gt_file']) for i in idxs])
            deps = np.stack([np.stack([hop_io.read_png(f) for f in ds['train'].samples[i]['depth_files']]) for i in idxs]).astype(np.uint16)
            tabs = [np.stack(x) for x in zip(*[A.build_tables(ds['train'].draw(3, 2, i), 128, 64, 64) for i in idxs])]
            out = (batch['inputs']['seg'], batch['labels']['seg'], batch['inputs']['depth'], batch['inputs']['depth_mask'])
            assert_same([o.cpu().numpy() for o in out], want(segs, labs, deps, tabs))
            assert batch['meta']['city'] == [ds['train'].samples[i]['city'] for i in idxs]
    val = D.NativeBatches(ds['val'], params, 0, 1, train=False, threads=2)
    (vb,) = list(val.batches(1))
    val.close()
    assert vb['inputs']['seg'].shape == (2, 3, 64, 128)
    assert np.array_equal(vb['labels']['seg'][1].cpu().numpy(), hop_io.read_png(ds['val'].samples[1]['gt_file']))


def test_train_driver_on_a_generated_tree(tmp_path):
    """train_bg.py --dataset native: 8 training samples, crop_size 64, two epochs with validation; the reference's checkpoint files
    appear, every value is finite, and 1 and 4 loader threads give bit-identical model_checkpoints."""
    from panoptic_forecasting_amd import train_bg
    root = str(tmp_path)
    cfg = os.path.join(root, 'cfg.yaml')
    tree_config(root, make_tree(root), cfg)
    sds = []
    for threads in (1, 4):
        wd = os.path.join(root, 'exp%d' % threads)
        train_bg.main(['--config_file', cfg, '--working_dir', wd, '--dataset', 'native',
                       '--extra_args', 'training.num_data_workers', str(threads)])
        for name in ('config.yaml', 'model_checkpoint', 'best_model', 'training_checkpoint'):
            assert os.path.exists(os.path.join(wd, name)), name
        st = torch.load(os.path.join(wd, 'training_checkpoint'))
        assert st['epoch'] == 3 and st['step'] == 8          # 2 epochs x 4 batches
        assert np.isfinite(st['best_val_result'])
        sd = torch.load(os.path.join(wd, 'model_checkpoint'))
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
        sds.append(sd)
    assert sds[0].keys() == sds[1].keys()
    for k in sds[0]:
        assert torch.equal(sds[0][k], sds[1][k]), k
