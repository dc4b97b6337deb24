#!/usr/bin/env python
"""Instance-AP records on one MI355X: prints one JSON line (kept as profiles/ap_bench.json).

    python tools/bench_ap.py [--batch 8] [--height 1024] [--width 2048] [--masks_per_image 12] [--reps 7] [--calls 20] [--host_reps 2]

Inputs: B seeded street scenes at 1024x2048: a road, a void band at the bottom (ego vehicle), a group of persons and
`masks_per_image` vehicles and persons as boxes of 40x20 to 400x300 pixels, written as a Cityscapes instance map; one predicted mask
per instance, its box moved and resized by a few per cent.  12 masks per image is what the project's own fg fixture holds
(tests/golden/g5_panoptic.npz: 23 instances in 2 images of 1024x2048).  Per ground-truth kind (u16, i32, i64), in one process,
repetition by repetition in turn:
  device_us        pf_ap_accumulate alone (fill + size + overlap + record + regular), device events around `calls` enqueued calls
  gpu_host_ms      instance_ap.records_host on the same device tensors (torch.bincount per mask; it reads values back, so it
                   synchronises: host clock around one call, the device idle before it)
  cpu_ms           instance_ap.records_host on host copies, host clock, one call per repetition
each reported as the median with every repetition listed, and
  size_us / overlap_us / record_us / regular_us   the four kernels from the library's event profiler (pf_profile_*); the overlap
                   pass with the byte rate it reaches on the mask bytes alone (P * H * W bytes: what no formulation can avoid
                   reading) and that rate's share of the HBM peak (8 TB/s).  It also reads its image's ground truth under every
                   mask (2 to 8 bytes per pixel and mask, the same map for all masks of an image: cache traffic, not HBM).
The three paths must agree (records and region counts equal) before they are timed.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from panoptic_forecasting_amd import instance_ap as ia, lib  # noqa: E402

HBM_PEAK = 8.0e12
GT_KIND = {'u16': 0, 'i32': 1, 'i64': 2}


def street_scenes(b, h, w, per_image, seed):
    """(gt [b,h,w] int64, masks [b*per_image,h,w] u8, mask_image, labels, scores)"""
    rng = np.random.default_rng(seed)
    gt = np.full((b, h, w), 7, np.int64)
    masks = np.zeros((b * per_image, h, w), np.uint8)
    image, labels = np.repeat(np.arange(b, dtype=np.int32), per_image), np.zeros(b * per_image, np.int32)
    gt[:, h - h // 8:] = 1                                            # ego vehicle: void
    for i in range(b):
        gt[i, h // 2:h // 2 + h // 16, w // 8:w // 4] = 24            # a group of persons
        for k in range(per_image):
            label = int(rng.choice([24, 24, 25, 26, 26, 26, 26, 27, 28, 32, 33]))
            bh, bw = int(rng.integers(20, max(21, h * 300 // 1024))), int(rng.integers(40, max(41, w * 400 // 2048)))
            y, x = int(rng.integers(h // 3, h - h // 8 - bh)), int(rng.integers(0, w - bw))
            gt[i, y:y + bh, x:x + bw] = label * 1000 + k
            dy, dx = int(rng.integers(-bh // 10 - 1, bh // 10 + 2)), int(rng.integers(-bw // 10 - 1, bw // 10 + 2))
            masks[i * per_image + k, max(0, y + dy):y + dy + bh, max(0, x + dx):x + dx + bw] = 1
            labels[i * per_image + k] = label
    return gt, masks, image, labels, rng.random(b * per_image)


def events_rep(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def host_rep(m, i, l, g, min_region):
    if m.is_cuda:
        torch.cuda.synchronize()
    t = time.perf_counter()
    ia.records_host(m, i, l, g, min_region)
    return (time.perf_counter() - t) * 1e3


def kernel_us(call, calls=10):
    lib.profile(True)
    for _ in range(calls):
        call()
    torch.cuda.synchronize()
    rows = lib.profile_results()
    lib.profile(False)
    out = {}
    for name in ('size', 'overlap', 'record', 'regular'):
        mine = [r for r in rows if 'ap_%s_kernel' % name in r['label']]
        out[name] = sum(r['ms'] for r in mine) / sum(r['launches'] for r in mine) * 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=1024)
    ap.add_argument('--width', type=int, default=2048)
    ap.add_argument('--masks_per_image', type=int, default=12)
    ap.add_argument('--min_region', type=int, default=100)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--host_reps', type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_ap: needs a GPU (a time taken anywhere else says nothing)')
    gt, masks, image, labels, scores = street_scenes(a.batch, a.height, a.width, a.masks_per_image, seed=5)
    L = lib.load()
    p = len(masks)
    res = {'metric': 'ap_accumulate', 'B': a.batch, 'H': a.height, 'W': a.width, 'P': p, 'masks_per_image': a.masks_per_image,
           'min_region': a.min_region, 'reps': a.reps, 'calls': a.calls, 'host_reps': a.host_reps,
           'library': os.path.basename(lib.LIB_PATH), 'chunk_pixels': L.pf_ap_chunk_pixels(), 'hbm_peak_tb_s': HBM_PEAK / 1e12,
           'mask_pixels_share': round(float((masks != 0).mean()), 5), 'gt': {}}
    hm, hi, hl = torch.from_numpy(masks), torch.from_numpy(image), torch.from_numpy(labels)
    m, i, l, s = hm.cuda(), hi.cuda(), hl.cuda(), torch.from_numpy(scores).cuda()
    for name in ('u16', 'i32', 'i64'):
        hg = (torch.from_numpy(gt.astype(np.uint16).view(np.int16)) if name == 'u16' else
              torch.from_numpy(gt).to(torch.int32 if name == 'i32' else torch.int64))
        g = hg.cuda()
        meter = ia.InstanceAP(a.min_region)
        rec, regular = meter.update(m, i, l, s, g)
        result = meter.result()
        gpu_rec, gpu_regular = ia.records_host(m, i, l, g, a.min_region)
        cpu_rec, cpu_regular = ia.records_host(hm, hi, hl, hg, a.min_region)
        assert torch.equal(rec.cpu(), gpu_rec) and torch.equal(regular.cpu(), gpu_regular), 'the kernels and the GPU torch formulation differ'
        assert torch.equal(rec.cpu(), cpu_rec) and torch.equal(regular.cpu(), cpu_regular), 'the kernels and the CPU formulation differ'
        ws = meter._ws
        call = lambda: lib.check(L.pf_ap_accumulate(m.data_ptr(), i.data_ptr(), l.data_ptr(), p, g.data_ptr(), GT_KIND[name], a.batch,
                                                    a.height, a.width, a.min_region, rec.data_ptr(), regular.data_ptr(), ws.data_ptr(),
                                                    ws.numel(), lib.stream_ptr()), 'pf_ap_accumulate')
        events_rep(call, 5)                                                        # warm-up
        dev_us, gpu_ms, cpu_ms = [], [], []
        for r in range(a.reps):                                                    # in turn, repetition by repetition
            dev_us.append(events_rep(call, a.calls))
            if r < a.host_reps:
                gpu_ms.append(host_rep(m, i, l, g, a.min_region))
                cpu_ms.append(host_rep(hm, hi, hl, hg, a.min_region))
        k = kernel_us(call)
        mask_bytes = float(p * a.height * a.width)
        d, q, c = (statistics.median(x) for x in (dev_us, gpu_ms, cpu_ms))
        res['gt'][name] = {
            'device_us': round(d, 2), 'device_us_reps': [round(x, 2) for x in dev_us],
            'gpu_host_ms': round(q, 2), 'gpu_host_ms_reps': [round(x, 2) for x in gpu_ms],
            'cpu_ms': round(c, 1), 'cpu_ms_reps': [round(x, 1) for x in cpu_ms],
            'speedup_vs_gpu_host': round(q * 1e3 / d, 1), 'speedup_vs_cpu': round(c * 1e3 / d, 1),
            'size_us': round(k['size'], 2), 'overlap_us': round(k['overlap'], 2), 'record_us': round(k['record'], 2),
            'regular_us': round(k['regular'], 2), 'mask_mb': round(mask_bytes / 1e6, 1),
            'mask_byte_floor_us': round(mask_bytes / HBM_PEAK * 1e6, 2),
            'overlap_mask_tb_s': round(mask_bytes / (k['overlap'] * 1e-6) / 1e12, 3),
            'overlap_share_of_mask_byte_floor': round(mask_bytes / HBM_PEAK * 1e6 / k['overlap'], 3),
            'allAp': result['allAp'], 'allAp50%': result['allAp50%'], 'regular_regions': int(regular.sum())}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
