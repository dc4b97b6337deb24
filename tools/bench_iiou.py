#!/usr/bin/env python
"""Instance-weighted IoU sums on one MI355X: prints one JSON line (kept as profiles/iiou_bench.json).

    python tools/bench_iiou.py [--batch 8] [--height 1024] [--width 2048] [--reps 7] [--calls 50] [--host_reps 3]

Inputs: B images from the test scene generator (tests/pq_scenes.py) scaled up to 1024x2048: the prediction reduced to classes (u8)
and the ground truth written as a Cityscapes instance map (tests/iiou_scenes.py), as u16, i32 and i64.  Per instance kind, in one
process, repetition by repetition in turn:
  device_us        pf_iiou_accumulate alone (fill + count + weigh + finish), device events around `calls` enqueued calls
  update_us        SemanticIoU.update(pred, gt, inst=...): the confusion call and the iIoU call together, the same way
  gpu_unique_ms    semantic_iou.instance_sums_host on the same device tensors (torch.unique per image; it reads values back, so it
                   synchronises: host clock around one call, the device idle before it)
  cpu_ms           semantic_iou.instance_sums_host on host copies of the maps, host clock, one call per repetition
each reported as the median with every repetition listed (the spread is theirs to show), and
  count_us / weigh_us / finish_us   the three kernels from the library's event profiler (pf_profile_*), the count pass with its
                   share of the byte floor: it has to read both maps once - 3 bytes per pixel for u8 + u16 - at the HBM peak
                   (8 TB/s).  Every timed call reads the same maps; the u8 + u16 / i32 ones fit the 256 MB Infinity Cache, so that
                   share is of the HBM peak RATE with the maps cache-resident
The three paths must agree (float64 pairs equal in bits, counts equal) before they are timed.
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import iiou_scenes as IS  # noqa: E402
from panoptic_forecasting_amd import lib, semantic_iou as si  # noqa: E402

HBM_PEAK = 8.0e12
INST_KIND = {'u16': 0, 'i32': 1, 'i64': 2}


def events_rep(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def host_rep(p, i):
    if p.is_cuda:
        torch.cuda.synchronize()
    t = time.perf_counter()
    si.instance_sums_host(p, i)
    return (time.perf_counter() - t) * 1e3


def kernel_us(call, calls=10):
    lib.profile(True)
    for _ in range(calls):
        call()
    torch.cuda.synchronize()
    rows = lib.profile_results()
    lib.profile(False)
    out = {}
    for name in ('count', 'weigh', 'finish'):
        mine = [r for r in rows if 'iiou_%s_kernel' % name in r['label']]
        out[name] = sum(r['ms'] for r in mine) / sum(r['launches'] for r in mine) * 1e3
    return out


def same_bits(a, b):
    return torch.equal(a.cpu().view(torch.int64), b.cpu().view(torch.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=1024)
    ap.add_argument('--width', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--host_reps', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_iiou: needs a GPU (a time taken anywhere else says nothing)')
    preds, gts, insts = IS.make_scenes(n=a.batch, h=a.height, w=a.width, seed=5)
    L = lib.load()
    res = {'metric': 'iiou_accumulate', 'B': a.batch, 'H': a.height, 'W': a.width, 'reps': a.reps, 'calls': a.calls,
           'host_reps': a.host_reps, 'library': os.path.basename(lib.LIB_PATH), 'chunk_pixels': L.pf_iiou_chunk_pixels(),
           'hbm_peak_tb_s': HBM_PEAK / 1e12, 'pred': 'u8', 'inst': {}}
    hp, hg = torch.from_numpy(preds).to(torch.uint8), torch.from_numpy(gts).to(torch.uint8)
    p, g = hp.cuda(), hg.cuda()
    for name in ('u16', 'i32', 'i64'):
        hi = (torch.from_numpy(insts.astype(np.uint16).view(np.int16)) if name == 'u16' else
              torch.from_numpy(insts).to(torch.int32 if name == 'i32' else torch.int64))
        i = hi.cuda()
        meter = si.SemanticIoU()
        per = torch.empty(a.batch, 8, 2, dtype=torch.float64, device='cuda')
        counts = torch.empty(a.batch, 8, 3, dtype=torch.int64, device='cuda')
        meter.update(p, g, inst=i, per_image_inst=per, per_image_inst_counts=counts)
        meter.result()
        gpu_sums, gpu_counts = si.instance_sums_host(p, i)
        cpu_sums, cpu_counts = si.instance_sums_host(hp, hi)
        assert same_bits(per, gpu_sums) and torch.equal(counts.cpu(), gpu_counts), 'the kernels and the GPU unique formulation differ'
        assert same_bits(per, cpu_sums) and torch.equal(counts.cpu(), cpu_counts), 'the kernels and the CPU formulation differ'
        ws = meter._ws_inst
        call = lambda: lib.check(L.pf_iiou_accumulate(p.data_ptr(), 0, i.data_ptr(), INST_KIND[name], 0, 19, a.batch, a.height, a.width,
                                                      meter.acc_inst.data_ptr(), meter.acc_inst_counts.data_ptr(), None, None,
                                                      ws.data_ptr(), ws.numel(), lib.stream_ptr()), 'pf_iiou_accumulate')
        update = lambda: meter.update(p, g, inst=i)
        events_rep(call, 5)                                                        # warm-up of every path
        events_rep(update, 5)
        dev_us, upd_us, gpu_ms, cpu_ms = [], [], [], []
        for r in range(a.reps):                                                    # in turn, repetition by repetition
            dev_us.append(events_rep(call, a.calls))
            upd_us.append(events_rep(update, a.calls))
            if r < a.host_reps:
                gpu_ms.append(host_rep(p, i))
                cpu_ms.append(host_rep(hp, hi))
        meter.result()
        k = kernel_us(call)
        map_bytes = float(a.batch * a.height * a.width * (p.element_size() + i.element_size()))
        floor_us = map_bytes / HBM_PEAK * 1e6
        d, u, q, c = (statistics.median(x) for x in (dev_us, upd_us, gpu_ms, cpu_ms))
        res['inst'][name] = {
            'device_us': round(d, 2), 'device_us_reps': [round(x, 2) for x in dev_us],
            'update_us': round(u, 2), 'update_us_reps': [round(x, 2) for x in upd_us],
            'gpu_unique_ms': round(q, 2), 'gpu_unique_ms_reps': [round(x, 2) for x in gpu_ms],
            'cpu_ms': round(c, 1), 'cpu_ms_reps': [round(x, 1) for x in cpu_ms],
            'speedup_vs_gpu_unique': round(q * 1e3 / d, 1), 'speedup_vs_cpu': round(c * 1e3 / d, 1),
            'instances': int(counts[:, :, 0].sum()), 'instance_pixels': int(counts[:, :, 1].sum()),
            'map_mb': round(map_bytes / 1e6, 1), 'byte_floor_us': round(floor_us, 2),
            'count_us': round(k['count'], 2), 'weigh_us': round(k['weigh'], 2), 'finish_us': round(k['finish'], 2),
            'count_tb_s': round(map_bytes / (k['count'] * 1e-6) / 1e12, 3), 'count_share_of_byte_floor': round(floor_us / k['count'], 3)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
