#!/usr/bin/env python
"""odometry forecaster latency / throughput on one MI355X: prints one JSON line.

    python tools/bench_odom.py [--sizes 1,32,512,12000] [--iters 50] [--reps 5] [--warmup 5] [--out FILE]

Per B (sequences; T_in = T_out = 9, the export's windows): us per forward and sequences/s for pf_odom_forward eager
(OdomModel.forward) and replayed from a captured graph, and the same forward as an eager torch fp32 restatement
(nn.GRU + nn.Linear from the same weights, the reference's OdomModel.forward op for op) on the same GPU.  The three are
timed in the same process, alternated rep by rep, and the median rep is reported.  ``frac_fp32_matrix_peak`` = the
forward's FLOPs (computed from the shapes: 2 * B * ((T_in - 1 + T_out) * 384 * (128 + 2) + T_out * 2 * 128)) over the
native graph-replayed time and the fp32 matrix peak (157.3 TFLOP/s).

    python tools/bench_odom.py --train [--sizes 32,1000,12000] ...

us per ``loss + backward`` (OdomModel.loss -> .mean().backward(): pf_odom_train_forward, the loss in torch ops,
pf_odom_backward, the accumulation into ``.grad``) against eager torch fp32 autograd of the same network and loss
(nn.GRU + nn.Linear from the same weights) on the same GPU, alternated rep by rep, median reported.  Gradients are set to
None before every call on both sides.
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import odom_ref64 as R  # noqa: E402
from panoptic_forecasting_amd.registry import build_model  # noqa: E402

PEAK_FP32_MATRIX = 157.3e12
T_IN = T_OUT = 9


class TorchOdom(nn.Module):
    """OdomModel.forward (odom_model.py:79-106) of the shipped config in eager torch ops."""

    def __init__(self, sd):
        super().__init__()
        self.rnn = nn.GRU(2, 128, batch_first=True)
        self.out = nn.Sequential(nn.Linear(128, 2))
        self.register_buffer('odom_mean', sd['odom_mean'].clone())
        self.register_buffer('odom_std', sd['odom_std'].clone())
        self.load_state_dict({k: v for k, v in sd.items()})

    @torch.no_grad()
    def forward(self, inps, output_len):
        return self.run(inps, output_len)

    def run(self, inps, output_len):
        inps = (inps - self.odom_mean) / self.odom_std
        _, hidden = self.rnn(inps[:, :-1])
        cur = inps[:, -1].unsqueeze(1)
        res = []
        for _ in range(output_len):
            out, hidden = self.rnn(cur, hidden)
            cur = self.out(out)
            res.append(cur)
        res = torch.cat(res, 1)
        return res * self.odom_std + self.odom_mean, res


def flops(b):
    return 2.0 * b * ((T_IN - 1 + T_OUT) * 384 * (128 + 2) + T_OUT * 2 * 128)


def time_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def train_main(args, model, ref):
    """us per loss + backward (mse on the normalised pair, the shipped config), native against eager torch autograd."""
    res = {'metric': 'odom_loss_backward', 'T_in': T_IN, 'T_out': T_OUT, 'device': torch.cuda.get_device_name(0), 'sizes': {}}
    mean, std = ref.odom_mean, ref.odom_std
    ref.train()                 # the RNN backward of the vendor library exists in training mode only (no dropout: same numbers)
    for b in [int(s) for s in (args.sizes or '32,1000,12000').split(',')]:
        x, y = R.make_inputs(1, b).cuda(), R.make_inputs(2, b).cuda()
        inputs, labels = {'odometry': x}, {'odometry': y}

        def native():
            for p in model.parameters():
                p.grad = None
            model.loss(inputs, labels)['loss'].mean().backward()

        def torch_fp32():
            for p in ref.parameters():
                p.grad = None
            _, norm = ref.run(x, T_OUT)
            loss = nn.functional.mse_loss(norm, (y - mean) / std, reduction='none')
            loss.reshape(b, -1).mean(1).mean().backward()
        for _ in range(args.warmup):
            native()
            torch_fp32()
        err = max(((p.grad - q.grad).abs().max() / q.grad.abs().max()).item()
                  for p, q in zip(list(model.parameters())[2:], ref.parameters()))
        runs = {'native': [], 'torch': []}
        for _ in range(args.reps):
            runs['native'].append(time_us(native, args.iters))
            runs['torch'].append(time_us(torch_fp32, args.iters))
        med = {k: statistics.median(v) for k, v in runs.items()}
        res['sizes'][str(b)] = {
            'native_us': round(med['native'], 2), 'torch_fp32_us': round(med['torch'], 2),
            'speedup_vs_torch_eager': round(med['torch'] / med['native'], 2),
            'spread_native_us': [round(min(runs['native']), 2), round(max(runs['native']), 2)],
            'spread_torch_us': [round(min(runs['torch']), 2), round(max(runs['torch']), 2)],
            'max_rel_grad_diff_vs_torch': err}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--train', action='store_true', help='time loss + backward instead of the forward')
    ap.add_argument('--sizes')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out')
    args = ap.parse_args()
    p = R.odom_params()
    p['no_gpu'] = False
    model = build_model(p)
    model.load_state_dict(R.fill_weights(model.state_dict()))
    ref = TorchOdom({k: v.detach() for k, v in model.state_dict().items()}).cuda().eval()
    if args.train:
        line = json.dumps(train_main(args, model, ref))
        print(line)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(line + '\n')
        return
    res = {'metric': 'odom_forward', 'T_in': T_IN, 'T_out': T_OUT, 'peak_fp32_matrix_tflops': PEAK_FP32_MATRIX / 1e12,
           'device': torch.cuda.get_device_name(0), 'sizes': {}}
    for b in [int(s) for s in (args.sizes or '1,32,512,12000').split(',')]:
        x = R.make_inputs(1, b).cuda()
        native = lambda: model(x, T_OUT)
        torch_fp32 = lambda: ref(x, T_OUT)
        for _ in range(args.warmup):
            native()
            torch_fp32()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            native()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cap, _ = model(x, T_OUT)
        g.replay()
        eager_out, _ = native()
        torch.cuda.synchronize()
        assert torch.equal(cap, eager_out), 'graph replay differs from eager'
        err = (eager_out - torch_fp32()[0]).abs().max().item()
        runs = {'eager': [], 'graph': [], 'torch': []}
        for _ in range(args.reps):
            runs['eager'].append(time_us(native, args.iters))
            runs['graph'].append(time_us(g.replay, args.iters))
            runs['torch'].append(time_us(torch_fp32, args.iters))
        med = {k: statistics.median(v) for k, v in runs.items()}
        res['sizes'][str(b)] = {
            'eager_us': round(med['eager'], 2), 'graph_us': round(med['graph'], 2), 'torch_fp32_us': round(med['torch'], 2),
            'eager_seq_per_s': round(b / med['eager'] * 1e6, 1), 'graph_seq_per_s': round(b / med['graph'] * 1e6, 1),
            'torch_seq_per_s': round(b / med['torch'] * 1e6, 1),
            'speedup_vs_torch_eager': round(med['torch'] / med['eager'], 2),
            'speedup_graph_vs_torch': round(med['torch'] / med['graph'], 2),
            'frac_fp32_matrix_peak': round(flops(b) / (med['graph'] * 1e-6) / PEAK_FP32_MATRIX, 4),
            'spread_eager_us': [round(min(runs['eager']), 2), round(max(runs['eager']), 2)],
            'spread_torch_us': [round(min(runs['torch']), 2), round(max(runs['torch']), 2)],
            'max_abs_diff_vs_torch': err}
        del g
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
