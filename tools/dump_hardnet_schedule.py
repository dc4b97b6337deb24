"""Dump the inference schedule (pf_debug_hardnet_schedule, no GPU) over a grid of networks, sizes, routes and options, one digest per
configuration: `python tools/dump_hardnet_schedule.py OUT.txt` writes `<configuration> <steps> <sha256 of the rows and formats>` lines,
`--time N` instead prints the milliseconds of N calls for FC-HarDNet-70 at B = 16, 1024 x 2048 through the stem route.  Two builds of
the library (PF_LIBPFHIP picks one) schedule alike exactly when their files are equal: profiles/hardnet_schedule_split.md."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

from panoptic_forecasting_amd import lib as pflib  # noqa: E402
from panoptic_forecasting_amd import packing, synth  # noqa: E402
from test_hardnet_schedule_host import schedule  # noqa: E402  (the caller of pf_debug_hardnet_schedule the tests use)

# (option, value, the library's default)
OPTIONS = [None, ('packed_acts', 0, 1), ('split_f16', 0, 1), ('range_guard', 0, 1), ('fuse_pool', 0, 1), ('fuse_upsample', 0, 1),
           ('fuse_front', 0, 1), ('fuse_pairs', 0, 1), ('fuse_pairs', 3, 1), ('share_s', 0, 1), ('share_s', 2, 1), ('fold_final', 0, 1),
           ('fold_final', 2, 1), ('fold_down', 0, 1), ('fold_down', 2, 1), ('fold_lo', 0, 1), ('fold_lo', 2, 1), ('valu_remainder', 0, 1),
           ('use_tuned_table', 0, 1), ('profile_tag_ops', 1, 0)]
# pf_debug_force_conv: every kind, conv_s4 also with three cout tiles and with a K split
FORCED = [(1, 0, 0, 0), (1, 4, 2, 0), (2, 2, 2, 4), (4, 2, 0, 0), (5, 2, 0, 0), (5, 3, 0, 0), (5, 3, 3, 0)]
HARDNET = [(1, 64, 128), (2, 96, 200), (4, 1024, 2048), (16, 1024, 2048), (8, 520, 1036)]


def nets():
    """[(name, blob, in_ch, n_cls, [(b, h, w, stem_t)])]"""
    from test_fold_down_host import down_net
    from test_fold_wide_host import lo_net
    from test_gpu_fold_wide import all_forms_net
    with open(os.path.join(ROOT, 'tests', 'golden', 'calib_seed1234.json')) as f:
        sd = synth.make_state_dict(seed=1234, calib=json.load(f))
    out = [('hardnet70', packing.pack_blob(sd, 36, 11), 36, 11, [(b, h, w, t) for b, h, w in HARDNET for t in (3, 0)])]
    g = lambda: torch.Generator().manual_seed(1)  # noqa: E731
    for name, (spec, P) in (('all_forms', all_forms_net(g())), ('down', down_net(g(), 16, 46, 96)), ('lo', lo_net(g(), 16, 46, 63))):
        out.append((name, packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P), spec.in_ch, spec.n_cls,
                    [(2, 16, 40, 0), (1, 32, 80, 0)]))
    return out


def main():
    L = pflib.load()
    if sys.argv[1] == '--time':
        name, blob, in_ch, n_cls, _ = nets()[0]
        t0 = time.perf_counter()
        for _ in range(int(sys.argv[2])):
            schedule(blob, in_ch, n_cls, 16, 1024, 2048, 1024, 2048, 3)
        print('%.1f' % ((time.perf_counter() - t0) * 1e3))
        return
    lines = []
    all_nets = nets()
    configs = [('default' if o is None else '%s=%d' % o[:2], o, None) for o in OPTIONS] + [('force=%d,%d,%d,%d' % f, None, f) for f in FORCED]
    for label, opt, force in configs:
        if opt:
            pflib.check(L.pf_set_option(opt[0].encode(), opt[1]), 'pf_set_option')
            pflib.profile(opt[0] == 'profile_tag_ops')      # (labels are made only while a profile is being recorded)
        if force:
            pflib.check(L.pf_debug_force_conv(*force), 'pf_debug_force_conv')
        for name, blob, in_ch, n_cls, cases in all_nets:
            for b, h, w, t in cases:
                key = '%s %s B%d %dx%d %s' % (label, name, b, h, w, 'stem' if t else 'dense')
                try:
                    fmt, rows = schedule(blob, in_ch, n_cls, b, h, w, h, w, t)
                    lines.append('%s %d %s' % (key, len(rows), hashlib.sha256(fmt.tobytes() + rows.tobytes()).hexdigest()))
                except pflib.PfError as e:
                    lines.append('%s refused: %s' % (key, str(e).split(': ', 1)[-1]))
        if opt:
            pflib.check(L.pf_set_option(opt[0].encode(), opt[2]), 'pf_set_option')
            pflib.profile(False)
        if force:
            pflib.check(L.pf_debug_force_conv(0, 0, 0, 0), 'pf_debug_force_conv')
    with open(sys.argv[1], 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('%d configurations' % len(lines))


if __name__ == '__main__':
    main()
