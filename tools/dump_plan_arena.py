"""Digest of everything plan creation packs (no GPU): `python tools/dump_plan_arena.py [LIBPFHIP.so]` prints, per network and option
setting, the float count and SHA-256 of the weight arena (pf_debug_plan_arena) and of the four fold regions (pf_debug_plan_tail, _down,
_wide with form 2 and 3).  Networks: the seeded FC-HarDNet-70 of the host tests (36 input channels, 11 classes) and the four pair_net
variants of tests/test_share_s_host.py; settings: normalize_ranges 0 and 1, each with the defaults and with share_s, fold_final, fold_down
and fold_lo at 0 and at 2.  `--time N [LIB]` instead prints the milliseconds of each of N pf_debug_plan_arena calls on FC-HarDNet-70.
Two builds of the library pack alike exactly when their outputs are equal, compared on one machine (the range normalisation goes through
log2 and lround): profiles/conv_pack_move.md.  The library is loaded directly, so one that lacks newer entry points can be dumped too."""
import ctypes
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (its HIP runtime must be mapped before the library's: lib.load)

from panoptic_forecasting_amd import lib as pflib  # noqa: E402
from panoptic_forecasting_amd import packing, synth  # noqa: E402

# (option, value, the library's default)
OPTIONS = [None] + [(name, v, 1) for name in ('share_s', 'fold_final', 'fold_down', 'fold_lo') for v in (0, 2)]
REGIONS = [('arena', 'pf_debug_plan_arena', ()), ('tail', 'pf_debug_plan_tail', ()), ('down', 'pf_debug_plan_down', ()),
           ('down3', 'pf_debug_plan_wide', (2,)), ('lo', 'pf_debug_plan_wide', (3,))]


def load(path):
    L = ctypes.CDLL(path)
    for name in ['pf_set_option', 'pf_last_error'] + [r[1] for r in REGIONS]:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = pflib.SIGNATURES[name]
    return L


def call(L, name, *args):
    if getattr(L, name)(*args) != 0:
        raise RuntimeError('%s: %s' % (name, L.pf_last_error().decode()))


def region(L, entry, lead, blob, in_ch, n_cls):
    buf = ctypes.create_string_buffer(blob, len(blob))
    n = ctypes.c_size_t()
    call(L, entry, *lead, buf, len(blob), in_ch, n_cls, None, 0, ctypes.byref(n), None, 0)
    out = np.zeros(n.value, dtype=np.float32)
    call(L, entry, *lead, buf, len(blob), in_ch, n_cls, out.ctypes.data, out.size, ctypes.byref(n), None, 0)
    return out


def nets():
    """[(name, blob, in_ch, n_cls)]"""
    from test_gpu_share_s import pair_net
    from test_share_s_host import test_share_and_add_packings_hold_the_consumers_weights_once as pairs
    with open(os.path.join(ROOT, 'tests', 'golden', 'calib_seed1234.json')) as f:
        sd = synth.make_state_dict(seed=1234, calib=json.load(f))
    out = [('hardnet70', packing.pack_blob(sd, 36, 11), 36, 11)]
    for c_odd, c_even, deep in pairs.pytestmark[0].args[1]:
        spec, P = pair_net(torch.Generator().manual_seed(c_even), 12, c_odd, c_even, deep)
        out.append(('pair_%d_%d_%s' % (c_odd, c_even, 'deep' if deep else 'flat'),
                    packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P), spec.in_ch, spec.n_cls))
    return out


def main():
    argv = sys.argv[1:]
    n_time = int(argv.pop(argv.index('--time') + 1)) if '--time' in argv else 0
    argv = [a for a in argv if a != '--time']
    L = load(argv[0] if argv else pflib.LIB_PATH)
    if n_time:
        _, blob, in_ch, n_cls = nets()[0]
        buf, n = ctypes.create_string_buffer(blob, len(blob)), ctypes.c_size_t()
        for _ in range(n_time):
            t0 = time.perf_counter()
            call(L, 'pf_debug_plan_arena', buf, len(blob), in_ch, n_cls, None, 0, ctypes.byref(n), None, 0)
            print('%.1f' % ((time.perf_counter() - t0) * 1e3))
        return
    for name, blob, in_ch, n_cls in nets():
        for norm in (0, 1):
            call(L, 'pf_set_option', b'normalize_ranges', norm)
            for opt in OPTIONS:
                if opt:
                    call(L, 'pf_set_option', opt[0].encode(), opt[1])
                for label, entry, lead in REGIONS:
                    r = region(L, entry, lead, blob, in_ch, n_cls)
                    print('%s normalize_ranges=%d %s %s %d %s' % (name, norm, 'default' if opt is None else '%s=%d' % opt[:2], label, r.size,
                                                                 hashlib.sha256(r.tobytes()).hexdigest()))
                if opt:
                    call(L, 'pf_set_option', opt[0].encode(), opt[2])
        call(L, 'pf_set_option', b'normalize_ranges', 1)


if __name__ == '__main__':
    main()
