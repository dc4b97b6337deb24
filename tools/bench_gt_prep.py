#!/usr/bin/env python
"""Ground-truth preparation on one MI355X: prints one JSON line (kept as profiles/gt_prep_bench.json).

    python tools/bench_gt_prep.py [--batch 8] [--height 1024] [--width 2048] [--reps 7] [--calls 50] [--host_reps 2]

Inputs: B synthetic street-like instance maps (tests/gtprep_scenes.py: blocks of stuff in long runs, rectangles of thing instances),
as u16, i32 and i64 maps.  Per kind, in one process, repetition by repetition in turn:
  device_us        GTPreparer.prepare with every output (fill + stream + finish), device events around `calls` enqueued calls into
                   the same output tensors
  upload_us        the batch's instance maps from pinned host memory to the device, device events around `calls` copies
  host_ms          gt_prep.prepare_host on the same maps, host clock, one call per repetition (u16 only: the host formulation
                   widens every kind to int64 first)
each reported as the median with every repetition listed, and
  stream_us / finish_us   the two kernels alone from the library's event profiler (pf_profile_*), the stream pass with its share of the
                   byte floor: it reads the map once and writes 5 bytes per pixel, at the HBM peak (8 TB/s).  Every timed call reads
                   the same maps and writes the same outputs; the u16 batch (117 MB) fits the 256 MB Infinity Cache, so that share is
                   of the HBM peak RATE with the data cache-resident.
The device result must equal the host formulation before anything is timed.
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
import gtprep_scenes as S  # noqa: E402
from panoptic_forecasting_amd import gt_prep, lib  # noqa: E402

HBM_PEAK = 8.0e12


def events_rep(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def kernel_us(fn, calls=10):
    lib.profile(True)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    rows = lib.profile_results()
    lib.profile(False)
    out = {}
    for name in ('stream', 'finish'):
        mine = [r for r in rows if 'gt_%s_kernel' % name in r['label']]
        out[name] = sum(r['ms'] for r in mine) / sum(r['launches'] for r in mine) * 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=1024)
    ap.add_argument('--width', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--host_reps', type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_gt_prep: needs a GPU (a time taken anywhere else says nothing)')
    maps = np.stack([S.blocky(a.height, a.width, 100 + i, n_things=90, block=64) for i in range(a.batch)])
    res = {'metric': 'gt_prepare', 'B': a.batch, 'H': a.height, 'W': a.width, 'reps': a.reps, 'calls': a.calls, 'host_reps': a.host_reps,
           'library': os.path.basename(lib.LIB_PATH), 'max_segments': gt_prep.max_segments(), 'hbm_peak_tb_s': HBM_PEAK / 1e12,
           'kinds': {}}
    host_maps = maps.astype(np.uint16)
    want = gt_prep.prepare_host(host_maps)
    res['segments_per_image'] = [int(x) for x in want['seg_count']]
    host_ms = []
    for _ in range(a.host_reps):
        t = time.perf_counter()
        gt_prep.prepare_host(host_maps)
        host_ms.append((time.perf_counter() - t) * 1e3)
    for name, dt in (('u16', np.int16), ('i32', np.int32), ('i64', np.int64)):
        hm = torch.from_numpy(host_maps.view(np.int16) if name == 'u16' else maps.astype(dt)).pin_memory()
        inst = hm.cuda()
        prep = gt_prep.GTPreparer('cuda')
        out = prep.prepare(inst)
        for k in ('panoptic', 'trainids', 'nofg', 'seg_count'):
            assert np.array_equal(out[k].cpu().numpy(), want[k]), 'the kernel and the host formulation differ in %s' % k
        assert all(np.array_equal(x, y) for x, y in zip(gt_prep.segment_rows(out), gt_prep.segment_rows(want))), 'segment rows differ'
        call = lambda: prep.prepare(inst, out=out, check=False)
        upload = lambda: inst.copy_(hm, non_blocking=True)
        events_rep(call, 5)
        events_rep(upload, 5)
        dev_us, up_us = [], []
        for _ in range(a.reps):
            dev_us.append(events_rep(call, a.calls))
            up_us.append(events_rep(upload, a.calls))
        prep.check()
        k = kernel_us(call)
        n = a.batch * a.height * a.width
        moved = n * (inst.element_size() + 5.0)
        floor_us = moved / HBM_PEAK * 1e6
        d = statistics.median(dev_us)
        res['kinds'][name] = {
            'device_us': round(d, 2), 'device_us_reps': [round(x, 2) for x in dev_us],
            'upload_us': round(statistics.median(up_us), 1), 'upload_us_reps': [round(x, 1) for x in up_us],
            'moved_mb': round(moved / 1e6, 1), 'byte_floor_us': round(floor_us, 2), 'stream_us': round(k['stream'], 2),
            'finish_us': round(k['finish'], 2), 'stream_tb_s': round(moved / (k['stream'] * 1e-6) / 1e12, 3),
            'stream_share_of_byte_floor': round(floor_us / k['stream'], 3)}
    h = statistics.median(host_ms)
    res['host_ms'] = round(h, 1)
    res['host_ms_reps'] = [round(x, 1) for x in host_ms]
    res['speedup_vs_host_u16'] = round(h * 1e3 / res['kinds']['u16']['device_us'], 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
