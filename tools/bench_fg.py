#!/usr/bin/env python
"""fg forecaster throughput on one MI355X: prints one JSON line.

    python tools/bench_fg.py [--sizes 8,32,128,512] [--iters 20] [--warmup 3]

Per N (instances; 3 input and 3 output steps): ms per forward and instances/s for pf_fg_forward eager and replayed from a
captured graph, and the same forward in ATen fp32 ops (tests/fg_ref64.forward64 with dtype float32) from the same weights
on the same GPU.  At N = 32 (and the largest N) the per-kernel times come from the library's hipEvent profiler
(pf_profile_*); the ConvLSTM kernel's rate is reported as a fraction of the fp32 matrix peak (157.3 TFLOP/s).
"""
import argparse
import contextlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import fg_ref64 as R  # noqa: E402
from panoptic_forecasting_amd import lib  # noqa: E402
from panoptic_forecasting_amd.registry import build_model  # noqa: E402

PEAK_FP32_MATRIX = 157.3e12


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernel_table(model, args):
    lib.profile(True)
    model(*args)
    torch.cuda.synchronize()
    rows = lib.profile_results()
    lib.profile(False)
    out = {}
    for r in rows:
        o = out.setdefault(r['label'], {'launches': 0, 'ms': 0.0, 'flops': 0.0})
        o['launches'] += r['launches']
        o['ms'] += r['ms']
        o['flops'] += r['flops']
    for o in out.values():
        o['tflops'] = o['flops'] / o['ms'] / 1e9 if o['ms'] else 0.0
        o['ms'] = round(o['ms'], 4)
        o['tflops'] = round(o['tflops'], 2)
        del o['flops']
    lstm = [r for r in rows if 'lstm' in r['label']]
    ms, fl = sum(r['ms'] for r in lstm), sum(r['flops'] for r in lstm)
    return out, (fl / (ms * 1e-3) / PEAK_FP32_MATRIX if ms else 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='8,32,128,512')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    p = R.fg_params()
    p['no_gpu'] = False
    with contextlib.redirect_stdout(sys.stderr):        # the registry announces the task on stdout: keep ONE line there
        model = build_model(p)
    model.load_state_dict(R.fill_weights(model.state_dict()))
    sd = {k: v.detach().float() for k, v in model.state_dict().items()}
    res = {'metric': 'fg_forward', 'T_in': 3, 'T_out': 3, 'peak_fp32_matrix_tflops': PEAK_FP32_MATRIX / 1e12, 'sizes': {}}
    sizes = [int(s) for s in a.sizes.split(',')]
    for n in sizes:
        inputs, labels = R.make_inputs(99, [n])
        args = tuple(x.cuda() if torch.is_tensor(x) else x for x in R.forward_args(inputs, labels))
        eager = timed(lambda: model(*args), a.iters, a.warmup)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            model(*args)
        torch.cuda.current_stream().wait_stream(s)
        with torch.cuda.graph(g):
            model(*args)
        graph = timed(g.replay, a.iters, a.warmup)
        with torch.no_grad():
            aten = timed(lambda: R.forward64(sd, *args, dtype=torch.float32), max(2, a.iters // 4), 1)
        row = {'eager_ms': round(eager, 3), 'graph_ms': round(graph, 3), 'aten_fp32_ms': round(aten, 3),
               'eager_inst_per_s': round(n / eager * 1e3, 1), 'graph_inst_per_s': round(n / graph * 1e3, 1),
               'aten_inst_per_s': round(n / aten * 1e3, 1), 'speedup_vs_aten': round(aten / graph, 2)}
        if n == 32 or n == sizes[-1]:
            row['kernels'], row['convlstm_frac_of_peak'] = kernel_table(model, args)
            row['convlstm_frac_of_peak'] = round(row['convlstm_frac_of_peak'], 3)
        res['sizes'][str(n)] = row
        del g
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
