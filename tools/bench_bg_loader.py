#!/usr/bin/env python
"""Native bg loader on one MI355X: the augmentation kernel alone and the loader's three stages; prints one JSON line.

    python tools/bench_bg_loader.py [--threads 1,4,8,16] [--batches 3] [--iters 50] [--reps 5] [--out FILE]

A tree of 8 training samples in the exported layout (3 label PNGs, 1 ground-truth PNG, 3 u16 depth PNGs each, 1024 x 2048) is
generated from a seed into a temporary directory: label maps are blocky class regions with 2 % pixel noise, depth codes a smooth
ramp with +-32 codes of noise and 20 % holes (what makes a PNG cheap or dear to inflate is its entropy; real exports lie between a
clean label map and a noisy depth map).

  kernel   pf_bg_augment alone at B = 8, T = 3, 1024 x 2048 -> 800 x 800, parameters drawn with scale in [0.5, 2.0]: device
           events around ``iters`` launches, median of ``reps``; ``bytes`` = what the algorithm must move, from the shapes:
           out pixels * (T + 1 u8 read + T u16 read + T + 1 u8 written + T f32 + T u8 mask written) + the tables;
  stages   per thread count, over ``batches`` batches of 8: decode = host clock around NativeBatches.decode (files -> pinned
           staging + tables), upload = device events on the side stream around its copies, augment = device events around the kernel
           and its table slices, and loader = host clock around a whole ``batches(epoch)`` pass ending in a synchronise;
           all in samples/s, against ``step_samples_per_s`` = 8 / 14.45 ms, what the training step consumes.
"""
import argparse
import json
import os
import random
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from panoptic_forecasting_amd import bg_augment as A  # noqa: E402
from panoptic_forecasting_amd import bg_dataset as D  # noqa: E402
from panoptic_forecasting_amd import hop_io  # noqa: E402

STEP_MS, BATCH, T, H, W, SIZE = 14.45, 8, 3, 1024, 2048, 800


def make_sample(root, dirs, i):
    g = np.random.RandomState(i)
    city, seq = 'bench', '%06d' % i
    coarse = g.randint(0, 11, (H // 64, W // 64)).astype(np.uint8)
    lab = np.kron(coarse, np.ones((64, 64), np.uint8))
    hop_io.write_png(os.path.join(root, 'gt', 'train', city, '%s_%s_000019_gtFine_labelTrainIds.png' % (city, seq)), lab)
    ramp = np.linspace(300.0, 40000.0, H)[:, None] * np.ones((1, W))
    for d in dirs:
        noisy = np.where(g.rand(H, W) < 0.02, g.randint(0, 11, (H, W)), lab).astype(np.uint8)
        hop_io.write_png(os.path.join(d, 'train', city, hop_io.LABEL_PNG % (city, seq, 19)), noisy)
        q = np.where(g.rand(H, W) < 0.2, 0, ramp + g.randint(-32, 33, (H, W))).astype(np.uint16)
        hop_io.write_png(os.path.join(d, 'train', city, hop_io.DEPTH_PNG % (city, seq, 19)), q)


def make_tree(root, n):
    dirs = [os.path.join(root, 'frame%d' % i) for i in range(T)]
    for d in dirs + [os.path.join(root, 'gt')]:
        os.makedirs(os.path.join(d, 'train', 'bench'), exist_ok=True)
    with ThreadPoolExecutor(min(n, D.MAX_THREADS)) as pool:
        list(pool.map(lambda i: make_sample(root, dirs, i), range(n)))
    files = [os.path.join(dp, f) for dp, _, fs in os.walk(root) for f in fs]
    return dirs, sum(os.path.getsize(f) for f in files) / n


def params_for(root, dirs, threads, steps):
    return {'seed': 1, 'data': {'data_dir': dirs, 'gt_dir': os.path.join(root, 'gt'), 'data_splits': ['train'], 'use_depths': True,
                                'depth_h5_path': os.path.join(root, 'depth_%s.h5'), 'min_depth': 0.1, 'max_depth': 200,
                                'only_background': True, 'crop_size': SIZE, 'scale_min': 0.5, 'scale_max': 2.0, 'gap_len': [3],
                                'depth_norm_params': [20.0, 15.0]},
            'training': {'batch_size': BATCH, 'num_data_workers': threads, 'steps_per_epoch': steps}}


def device_ms(fn, iters, stream=None):
    """ms per call of ``fn`` between two events on ``stream`` (the stream ``fn`` enqueues on; default: the current one)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = stream or torch.cuda.current_stream()
    torch.cuda.synchronize()
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def bench_kernel(iters, reps, warmup=5):
    g = torch.Generator().manual_seed(0)
    seg = torch.randint(0, 19, (BATCH, T, H, W), generator=g, dtype=torch.uint8).cuda()
    lab = torch.randint(0, 19, (BATCH, H, W), generator=g, dtype=torch.uint8).cuda()
    dep = torch.randint(0, 32768, (BATCH, T, H, W), generator=g, dtype=torch.int16).cuda()
    tabs = [np.stack(x) for x in zip(*[A.build_tables(A.draw_params(random.Random(i), W, H, SIZE, 0.5, 2.0), W, H, SIZE)
                                       for i in range(BATCH)])]
    tabs = [torch.from_numpy(x).cuda() for x in tabs]
    out = A.device_augment(seg, lab, dep, *tabs, 0.1, 200.0)
    out = (out[0], out[1], out[2], out[3].view(torch.uint8))
    fn = lambda: A.device_augment(seg, lab, dep, *tabs, 0.1, 200.0, out=out)     # noqa: E731
    for _ in range(warmup):
        fn()
    ms = [device_ms(fn, iters) for _ in range(reps)]
    px = BATCH * SIZE * SIZE
    nbytes = px * ((T + 1) * 1 + T * 2 + (T + 1) * 1 + T * 4 + T * 1) + 4 * BATCH * 4 * SIZE
    med = statistics.median(ms)
    return {'ms': round(med, 4), 'spread_ms': [round(min(ms), 4), round(max(ms), 4)], 'bytes': nbytes,
            'gb_per_s': round(nbytes / med / 1e6, 1), 'samples_per_s': round(BATCH / med * 1e3, 1)}


def bench_stages(root, dirs, threads, batches):
    params = params_for(root, dirs, threads, batches)
    ds = D.build_dataset(params)['train']
    loader = D.NativeBatches(ds, params, 0, 1, train=True)
    loader._setup()
    plan = loader.index_batches(1)
    slot = loader._slots[0]
    loader.decode(slot, plan[0], 1)             # warm: file cache, pool threads
    t0 = time.perf_counter()
    for idxs in plan:
        loader.decode(slot, idxs, 1)
    decode_s = time.perf_counter() - t0
    loader.upload(slot)
    loader.augment(slot)
    up = device_ms(lambda: loader.upload(slot), 10, loader._stream)
    au = device_ms(lambda: loader.augment(slot), 20)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for batch in loader.batches(2):
        n += batch['inputs']['seg'].shape[0]
    torch.cuda.synchronize()
    total_s = time.perf_counter() - t0
    loader.close()
    return {'decode_samples_per_s': round(len(plan) * BATCH / decode_s, 1), 'upload_samples_per_s': round(BATCH / up * 1e3, 1),
            'upload_ms': round(up, 3), 'augment_samples_per_s': round(BATCH / au * 1e3, 1), 'augment_ms': round(au, 3),
            'loader_samples_per_s': round(n / total_s, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--threads', default='1,4,8,16')
    ap.add_argument('--batches', type=int, default=3)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_bg_loader.py measures on the GPU: none found')
    root = tempfile.mkdtemp(prefix='bg_loader_')
    try:
        dirs, bytes_per_sample = make_tree(root, BATCH)
        res = {'metric': 'bg_loader', 'batch': BATCH, 'source': [H, W], 'size': SIZE, 'T': T,
               'png_bytes_per_sample': int(bytes_per_sample), 'step_samples_per_s': round(BATCH / STEP_MS * 1e3, 1), 'threads': {}}
        res['device'] = torch.cuda.get_device_name(0)
        res['kernel'] = bench_kernel(args.iters, args.reps)
        for th in [int(x) for x in args.threads.split(',')]:
            res['threads'][str(th)] = bench_stages(root, dirs, th, args.batches)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
