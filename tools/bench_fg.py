#!/usr/bin/env python
"""fg forecaster throughput on one MI355X: prints one JSON line.

    python tools/bench_fg.py [--sizes 8,32,128,512] [--iters 20] [--warmup 3] [--arithmetic fp32|fp16_pair|both] [--reps 5]

Per N (instances; 3 input and 3 output steps): ms per forward and instances/s for pf_fg_forward eager and replayed from a
captured graph, and the same forward in ATen fp32 ops (tests/fg_ref64.forward64 with dtype float32) from the same weights
on the same GPU.  At N = 32 (and the largest N) the per-kernel times come from the library's hipEvent profiler
(pf_profile_*); the ConvLSTM kernel's rate is reported as a fraction of the fp32 matrix peak (157.3 TFLOP/s).

--arithmetic picks model.fg_arithmetic.  ``both`` builds one model per arithmetic in this process and, per N, times the two captured
forwards alternately, --reps windows of --iters replays each: per arithmetic the median window and the spread (min, max) of its
windows, so the two are compared on the same box in the same job.  ``pair_faster`` says whether the pair median lies below the fp32
median by more than the two spreads together.  The pair forward's ConvLSTM rate is fp32-EQUIVALENT work (one product per operand
pair) over kernel time; its share of the forward is the kernels' time over the sum of all kernels' times.  With --append FILE the
result is added to that JSON file under the key --key (the file's other keys are kept).
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
    total = sum(r['ms'] for r in rows)
    return out, (fl / (ms * 1e-3) / PEAK_FP32_MATRIX if ms else 0.0), (fl / (ms * 1e-3) / 1e12 if ms else 0.0), (ms / total if total else 0.0)


def captured(model, args):
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model(*args)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        model(*args)
    return g


def compare(models, sizes, iters, warmup, reps):
    """{N: {arithmetic: {graph_ms_median, graph_ms_min, graph_ms_max, windows}, pair_faster}}: alternating windows of captured replays"""
    out = {}
    for n in sizes:
        inputs, labels = R.make_inputs(99, [n])
        args = tuple(x.cuda() if torch.is_tensor(x) else x for x in R.forward_args(inputs, labels))
        graphs = {k: captured(m, args) for k, m in models.items()}
        for g in graphs.values():
            timed(g.replay, 1, warmup)
        windows = {k: [] for k in models}
        for _ in range(reps):
            for k, g in graphs.items():
                windows[k].append(timed(g.replay, iters, 0))
        row = {}
        for k, w in windows.items():
            w = sorted(w)
            row[k] = {'graph_ms_median': round(w[len(w) // 2], 3), 'graph_ms_min': round(w[0], 3), 'graph_ms_max': round(w[-1], 3),
                      'windows': len(w), 'status': models[k].fg_status()}
        if len(row) == 2:
            a, b = row['fp32'], row['fp16_pair']
            spread = (a['graph_ms_max'] - a['graph_ms_min']) + (b['graph_ms_max'] - b['graph_ms_min'])
            row['pair_over_fp32'] = round(b['graph_ms_median'] / a['graph_ms_median'], 3)
            row['pair_faster'] = bool(a['graph_ms_median'] - b['graph_ms_median'] > spread)
        if n == 32 or n == sizes[-1]:
            for k, m in models.items():
                table, frac, tflops, share = kernel_table(m, args)
                row[k].update(kernels=table, convlstm_tflops_fp32_equivalent=round(tflops, 1), convlstm_frac_of_fp32_peak=round(frac, 3),
                              convlstm_share_of_kernel_time=round(share, 3))
        out[str(n)] = row
        del graphs
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='8,32,128,512')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--arithmetic', choices=('fp32', 'fp16_pair', 'both'), default='fp32')
    ap.add_argument('--reps', type=int, default=5, help='both: timed windows per arithmetic and size')
    ap.add_argument('--append', help='JSON file to add the result to')
    ap.add_argument('--key', default='fg_arithmetic', help='key of the result in --append')
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(',')]

    def make(arithmetic):
        p = R.fg_params(fg_arithmetic=arithmetic, fg_on_range='ignore')      # nothing re-runs inside a timed window; the status is reported
        p['no_gpu'] = False
        with contextlib.redirect_stdout(sys.stderr):        # the registry announces the task on stdout: keep ONE line there
            m = build_model(p)
        m.load_state_dict(R.fill_weights(m.state_dict()))
        return m

    if a.arithmetic == 'both':
        res = {'metric': 'fg_forward_arithmetic', 'T_in': 3, 'T_out': 3, 'iters': a.iters, 'reps': a.reps,
               'peak_fp32_matrix_tflops': PEAK_FP32_MATRIX / 1e12,
               'sizes': compare({'fp32': make('fp32'), 'fp16_pair': make('fp16_pair')}, sizes, a.iters, a.warmup, a.reps)}
        finish(res, a)
        return
    model = make(a.arithmetic)
    sd = {k: v.detach().float() for k, v in model.state_dict().items()}
    res = {'metric': 'fg_forward', 'arithmetic': a.arithmetic, 'T_in': 3, 'T_out': 3, 'peak_fp32_matrix_tflops': PEAK_FP32_MATRIX / 1e12, 'sizes': {}}
    for n in sizes:
        inputs, labels = R.make_inputs(99, [n])
        args = tuple(x.cuda() if torch.is_tensor(x) else x for x in R.forward_args(inputs, labels))
        eager = timed(lambda: model(*args), a.iters, a.warmup)
        g = captured(model, args)
        graph = timed(g.replay, a.iters, a.warmup)
        with torch.no_grad():
            aten = timed(lambda: R.forward64(sd, *args, dtype=torch.float32), max(2, a.iters // 4), 1)
        row = {'eager_ms': round(eager, 3), 'graph_ms': round(graph, 3), 'aten_fp32_ms': round(aten, 3),
               'eager_inst_per_s': round(n / eager * 1e3, 1), 'graph_inst_per_s': round(n / graph * 1e3, 1),
               'aten_inst_per_s': round(n / aten * 1e3, 1), 'speedup_vs_aten': round(aten / graph, 2)}
        if n == 32 or n == sizes[-1]:
            row['kernels'], row['convlstm_frac_of_peak'] = kernel_table(model, args)[:2]
            row['convlstm_frac_of_peak'] = round(row['convlstm_frac_of_peak'], 3)
        res['sizes'][str(n)] = row
        del g
        torch.cuda.empty_cache()
    finish(res, a)


def finish(res, a):
    print(json.dumps(res))
    if a.append:
        data = {}
        if os.path.exists(a.append):
            with open(a.append) as f:
                data = json.load(f)
        data[a.key] = res
        with open(a.append, 'w') as f:
            json.dump(data, f)
            f.write('\n')


if __name__ == '__main__':
    main()
