#!/usr/bin/env python
"""Semantic confusion counting on one MI355X: prints one JSON line (kept as profiles/miou_bench.json).

    python tools/bench_miou.py [--batch 8] [--height 1024] [--width 2048] [--reps 7] [--calls 50]

Inputs: B images from the test scene generator (tests/pq_scenes.py) scaled up to 1024x2048 and reduced to classes
(tests/conf_scenes.py), as u8, i32 and i64 maps.  Per dtype, in one process, repetition by repetition in turn:
  device_us        SemanticIoU.update (fill + count + finish), device events around `calls` enqueued calls
  gpu_bincount_us  semantic_iou.confusion_host on the same device tensors (LUT gathers + torch.bincount), device events around
                   `calls` calls; the value check of that function synchronises, the time includes it as a caller pays it
  cpu_ms           semantic_iou.confusion_host on host copies of the maps, host clock, one call per repetition
each reported as the median with every repetition listed (the spread is theirs to show), and
  count_us         the count pass alone from the library's event profiler (pf_profile_*), with its share of the byte floor: the
                   pass has to read both maps once - 2 bytes per pixel for u8 - at the HBM peak (8 TB/s).  Every timed call
                   reads the same maps; the u8 and i32 ones fit the 256 MB Infinity Cache, so that share is of the HBM peak RATE
                   with the maps cache-resident
The three paths must agree (integer tables, equal) before they are timed.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import conf_scenes as CS  # noqa: E402
from panoptic_forecasting_amd import lib, semantic_iou as si  # noqa: E402

HBM_PEAK = 8.0e12


def events_rep(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def cpu_rep(p, g):
    t = time.perf_counter()
    si.confusion_host(p, g)
    return (time.perf_counter() - t) * 1e3


def count_kernel_us(meter, p, g, calls=10):
    lib.profile(True)
    for _ in range(calls):
        meter.update(p, g)
    torch.cuda.synchronize()
    rows = [r for r in lib.profile_results() if 'conf_count_kernel' in r['label']]
    lib.profile(False)
    return sum(r['ms'] for r in rows) / sum(r['launches'] for r in rows) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=1024)
    ap.add_argument('--width', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--calls', type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_miou: needs a GPU (a time taken anywhere else says nothing)')
    preds, gts = CS.make_scenes(n=a.batch, h=a.height, w=a.width, seed=5)
    res = {'metric': 'confusion_accumulate', 'B': a.batch, 'H': a.height, 'W': a.width, 'reps': a.reps, 'calls': a.calls,
           'chunk_pixels': lib.load().pf_confusion_chunk_pixels(), 'hbm_peak_tb_s': HBM_PEAK / 1e12, 'dtypes': {}}
    for name, dt in (('u8', torch.uint8), ('i32', torch.int32), ('i64', torch.int64)):
        hp, hg = torch.from_numpy(preds).to(dt), torch.from_numpy(gts).to(dt)
        p, g = hp.cuda(), hg.cuda()
        meter = si.SemanticIoU()
        meter.update(p, g)
        meter.result()
        assert torch.equal(meter.acc, si.confusion_host(p, g)), 'the kernel and the GPU bincount formulation differ'
        assert torch.equal(meter.acc.cpu(), si.confusion_host(hp, hg)), 'the kernel and the CPU formulation differ'
        events_rep(lambda: meter.update(p, g), 5)                                # warm-up of all three paths
        events_rep(lambda: si.confusion_host(p, g), 5)
        cpu_rep(hp, hg)
        dev_us, bin_us, cpu_ms = [], [], []
        for _ in range(a.reps):                                                   # in turn, repetition by repetition
            dev_us.append(events_rep(lambda: meter.update(p, g), a.calls))
            bin_us.append(events_rep(lambda: si.confusion_host(p, g), a.calls))
            cpu_ms.append(cpu_rep(hp, hg))
        meter.result()
        count_us = count_kernel_us(meter, p, g)
        map_bytes = 2.0 * a.batch * a.height * a.width * p.element_size()
        floor_us = map_bytes / HBM_PEAK * 1e6
        d, q, c = statistics.median(dev_us), statistics.median(bin_us), statistics.median(cpu_ms)
        res['dtypes'][name] = {
            'device_us': round(d, 2), 'device_us_reps': [round(x, 2) for x in dev_us],
            'gpu_bincount_us': round(q, 1), 'gpu_bincount_us_reps': [round(x, 1) for x in bin_us],
            'cpu_ms': round(c, 1), 'cpu_ms_reps': [round(x, 1) for x in cpu_ms],
            'speedup_vs_gpu_bincount': round(q / d, 1), 'slowest_device_over_fastest_bincount': round(max(dev_us) / min(bin_us), 4),
            'speedup_vs_cpu': round(c * 1e3 / d, 1),
            'map_mb': round(map_bytes / 1e6, 1), 'byte_floor_us': round(floor_us, 2), 'count_us': round(count_us, 2),
            'count_tb_s': round(map_bytes / (count_us * 1e-6) / 1e12, 3), 'count_share_of_byte_floor': round(floor_us / count_us, 3)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
