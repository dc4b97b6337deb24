#!/usr/bin/env python
"""Native fg export loader on one MI355X: its stages and the forward it feeds; prints one JSON line.

    python tools/bench_fg_loader.py [--instances 12] [--rows 36] [--reps 7] [--calls 20] [--out FILE]

A tree of 8 scenes in the ``.npz``-twin layout (tests/fgscene_tree.py: 1024 x 2048 backgrounds, ``--instances`` instances per scene
over ``--rows`` feature rows per scene, the shipped mid-term configuration) is generated from a seed into a temporary directory.
At the shipped batch size (2 scenes) and at 8, after one warm-up pass over every shape:

  stage     host clock around NativeFGSceneDataset.stage_pinned: numpy selection, the scenes' feature rows into the pinned buffer
            (the twin route inflates a scene's whole feature dataset), the background PNGs decoded            median of ``reps``
  upload    host clock around upload() ending in a synchronise: tables, feature rows, u8 backgrounds           median of ``reps``
  kernel    pf_fg_assemble alone: the library's event pair around each of ``calls`` launches (lib.profile); ``gather_bytes`` =
            (N * T_in planes written + the planes that have a row, read) * 200 704, what the gather must move, and
            ``gather_gb_per_s`` = that over the kernel's time - an upper statement of the copy's cost, since the kernel's
            per-instance part and the event pair's own overhead are in the time; ``share_of_hbm`` against 6.29 TB/s, the
            measured float4-copy rate of MI355X_MICROARCH.md
  predict   host clock around FGModel.predict_panoptic of the assembled batch ending in a synchronise          median of ``reps``
  kernel_large  the kernel at N = 1024 over M = 256 rows (1.2 GB moved): the copy loop where launch overheads no longer count

Whether the loader or the forward bounds the export is what this records; no bar is set on it.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import fg_ref64 as R  # noqa: E402
import fgscene_tree as FT  # noqa: E402
from panoptic_forecasting_amd import fg_dataset as D  # noqa: E402
from panoptic_forecasting_amd import lib  # noqa: E402
from panoptic_forecasting_amd.registry import build_model  # noqa: E402

SCENES, HBM_TB_S, PLANE_BYTES = 8, 6.29, 200704
LABEL = 'pf::fg_assemble_kernel(pf::FgAsmArgs)'


def host_ms(fn, reps):
    """Median host-clock ms of ``fn`` + a device synchronise, and the spread."""
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return {'ms': round(statistics.median(ms), 3), 'spread_ms': [round(min(ms), 3), round(max(ms), 3)]}


def kernel_ms(fn, calls):
    lib.profile(True)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    rows = [r for r in lib.profile_results() if r['label'] == LABEL]
    lib.profile(False)
    launches = sum(r['launches'] for r in rows)
    if launches != calls:
        raise SystemExit('bench_fg_loader: expected %d launches of %s, the profile holds %d' % (calls, LABEL, launches))
    return sum(r['ms'] for r in rows) / launches


def kernel_entry(dev, kw, calls, warmup=3):
    n, t_in = dev['feat_row'].shape
    for _ in range(warmup):
        D.device_assemble(**dev, **kw)
    ms = kernel_ms(lambda: D.device_assemble(**dev, **kw), calls)
    valid = int(((dev['feat_row'] >= 0) & (dev['feat_row'] < dev['feat_table'].shape[0])).sum())
    nbytes = (n * t_in + valid) * PLANE_BYTES              # every plane is written; a plane without a row is not read
    gbs = nbytes / ms / 1e6 if n else 0.0
    return {'ms': round(ms, 5), 'instances': n, 'gather_bytes': nbytes, 'gather_gb_per_s': round(gbs, 1),
            'share_of_hbm': round(gbs / (HBM_TB_S * 1e3), 4)}


def bench_batch(ds, model, bs, reps, calls):
    idx = range(bs)
    batch = ds.device_batch(idx)                            # warm: file cache, pinned buffers, code objects
    with torch.no_grad():
        model.predict_panoptic(batch['inputs'], batch['labels'])
    torch.cuda.synchronize()
    out = {'stage': host_ms(lambda: ds.stage_pinned(idx), reps)}
    st = ds.stage_pinned(idx)
    out['upload'] = host_ms(lambda: ds.upload(st), reps)
    out['upload']['bytes'] = int(st['feat_table'].nbytes + (bs * 1024 * 2048 if st['has_background'] else 0))
    dev, _, _ = ds.upload(st)
    out['kernel'] = kernel_entry(dev, ds.assemble_kwargs(), calls)
    with torch.no_grad():
        out['predict'] = host_ms(lambda: model.predict_panoptic(batch['inputs'], batch['labels']), reps)
    out['loader_ms'] = round(out['stage']['ms'] + out['upload']['ms'] + out['kernel']['ms'], 3)
    out['bound_by'] = 'loader' if out['loader_ms'] > out['predict']['ms'] else 'forward'
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', type=int, default=12)
    ap.add_argument('--rows', type=int, default=36)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_fg_loader.py measures on the GPU: none found')
    root = tempfile.mkdtemp(prefix='fg_loader_')
    try:
        _, data = FT.write_synthetic(root, n_scenes=SCENES, seed=0, n_inst=args.instances, rows=args.rows)
        ds = D.NativeFGSceneDataset(FT.SPLIT, {'data': data}, test=True)
        params = R.fg_params(use_depth_sorting=True)
        params['no_gpu'] = False
        model = build_model(params)
        model.load_state_dict(R.fill_weights(model.state_dict()))
        model.eval()
        res = {'metric': 'fg_loader', 'device': torch.cuda.get_device_name(0), 'scenes': SCENES, 'instances_per_scene': args.instances,
               'feature_rows_per_scene': args.rows, 'files': 'npz twins', 'hbm_tb_per_s': HBM_TB_S, 'batches': {}}
        for bs in (2, 8):
            res['batches'][str(bs)] = bench_batch(ds, model, bs, args.reps, args.calls)
        big = {k: torch.from_numpy(v).cuda() for k, v in FT.random_tables(1024, 256, seed=1).items()}
        res['kernel_large'] = kernel_entry(big, {'use_ulbr': False, 'max_depth': None, 'filter_car_gap': None}, args.calls)
        ds.close()
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
