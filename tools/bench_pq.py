#!/usr/bin/env python
"""Panoptic-quality matching on one MI355X: prints one JSON line (kept as profiles/pq_bench.json).

    python tools/bench_pq.py [--batch 8] [--height 1024] [--width 2048] [--reps 5] [--calls 50]

Inputs: B images from the test scene generator (tests/pq_scenes.py) scaled up to 1024x2048, as i32 and as i64 maps
(16.8 / 33.6 MB per image for the two maps).  Per dtype:
  device_ms   PanopticQuality.update (crowd=True, the default), device events around `calls` enqueued calls, median of `reps` repetitions
  parent_ms   pq.pq_accumulate_panoptic on the same tensors, host clock around one call ending in a synchronise (the function
              synchronises once per image by itself), one call per repetition, alternating with the device repetitions
  count_us    the count pass alone from the library's event profiler (pf_profile_*), and its share of the HBM peak (8 TB/s): the
              pass is bound by reading the two maps once.  Every timed call reads the same maps: the i32 ones (134 MB at the default size) fit the
              256 MB Infinity Cache, so that share is of the HBM peak RATE with the maps cache-resident; the i64 ones do not fit
The two paths must agree before they are timed (counts equal, sum_iou to 1e-12).
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
import pq_scenes as S  # noqa: E402
from panoptic_forecasting_amd import lib, pq  # noqa: E402

HBM_PEAK = 8.0e12


def device_rep(meter, p, g, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        meter.update(p, g)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def parent_rep(p, g):
    torch.cuda.synchronize()
    t = time.perf_counter()
    pq.pq_accumulate_panoptic(p, g, 19)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def kernel_times(meter, p, g, calls=10):
    lib.profile(True)
    for _ in range(calls):
        meter.update(p, g)
    torch.cuda.synchronize()
    rows = lib.profile_results()
    lib.profile(False)
    out = {}
    for r in rows:
        o = out.setdefault(r['label'], {'launches': 0, 'ms': 0.0, 'bytes': 0.0})
        o['launches'] += r['launches']
        o['ms'] += r['ms']
        o['bytes'] += r['bytes']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=1024)
    ap.add_argument('--width', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--calls', type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_pq: needs a GPU (a time taken anywhere else says nothing)')
    preds, gts = S.make_scenes(n=a.batch, h=a.height, w=a.width, seed=5)
    res = {'metric': 'pq_accumulate', 'crowd': True, 'B': a.batch, 'H': a.height, 'W': a.width, 'reps': a.reps, 'calls': a.calls,
           'table_slots': lib.load().pf_pq_table_slots(), 'hbm_peak_tb_s': HBM_PEAK / 1e12, 'dtypes': {}}
    for name, dt in (('i32', torch.int32), ('i64', torch.int64)):
        p, g = torch.from_numpy(preds).to('cuda', dt), torch.from_numpy(gts).to('cuda', dt)
        meter = pq.PanopticQuality(19, 'trainid', crowd=True)                    # the timed setting: the default and the driver's
        meter.update(p, g)
        meter.result()
        gv = torch.where((g >= 11) & (g < 19), torch.full_like(g, 255), g)      # the parent has no crowd rule: compare without
        pv = torch.where((p >= 11) & (p < 19), torch.full_like(p, 255), p)
        new = pq.PanopticQuality(19, 'trainid', crowd=False).update(pv, gv)
        new.result()
        old = pq.pq_accumulate_panoptic(pv, gv, 19)
        assert torch.equal(new.acc[:, 1:], old[:, 1:]), 'counts differ from pq_accumulate_panoptic'
        assert ((new.acc[:, 0] - old[:, 0]).abs() <= 1e-12 * old[:, 0].abs()).all(), 'sum_iou differs from pq_accumulate_panoptic'
        device_rep(meter, p, g, 5)                                                # warm-up of both paths
        parent_rep(p, g)
        dev_ms, par_ms = [], []
        for _ in range(a.reps):                                                   # alternate the two, repetition by repetition
            dev_ms.append(device_rep(meter, p, g, a.calls))
            par_ms.append(parent_rep(p, g))
        meter.result()
        kt = kernel_times(meter, p, g)
        count = [v for k, v in kt.items() if 'pq_count_kernel' in k][0]
        count_us = count['ms'] / count['launches'] * 1e3
        map_bytes = 2.0 * a.batch * a.height * a.width * (4 if dt == torch.int32 else 8)
        d, q = statistics.median(dev_ms), statistics.median(par_ms)
        res['dtypes'][name] = {
            'device_ms': round(d, 4), 'device_ms_reps': [round(x, 4) for x in dev_ms],
            'parent_ms': round(q, 2), 'parent_ms_reps': [round(x, 2) for x in par_ms], 'speedup_vs_parent': round(q / d, 1),
            'map_mb': round(map_bytes / 1e6, 1), 'count_us': round(count_us, 2),
            'count_tb_s': round(map_bytes / (count_us * 1e-6) / 1e12, 3),
            'count_share_of_hbm_peak': round(map_bytes / (count_us * 1e-6) / HBM_PEAK, 3),
            'kernels_us': {k: round(v['ms'] / v['launches'] * 1e3, 2) for k, v in kt.items()},
            'distinct_pairs_max': int(max(len(np.unique(gts[b].ravel() * 65536 + preds[b].ravel())) for b in range(a.batch)))}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
