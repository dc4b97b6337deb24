"""Which kernel and tile shape a convolution gets (csrc/conv_select.cpp: decide_conv, s4_resolve), through
pf_debug_conv_decision: host code only, no GPU.

The golden (tests/golden/conv_decision.json) was recorded from the schedule's own logic BEFORE it moved into decide_conv:
commit 83472fd with pf_debug_conv_decision placed over a verbatim copy of the inference schedule's `choose` lambda and of
launch_conv_s4's ladder.  `python tests/test_conv_decision_host.py FILE` writes what the loaded library answers to FILE."""
import ctypes
import itertools
import json
import os
import sys

import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
else:
    from conftest import GOLDEN
from panoptic_forecasting_amd import hardnet_arch as arch
from panoptic_forecasting_amd import lib as pflib

GENERIC, SPLIT_PACK, S4_PACK, TUNED, SPLIT_F16, KACC = 1, 2, 4, 8, 16, 32   # `flags` of pf_debug_conv_decision (include/pfhip.h)
FIELDS = ('kind', 'p0', 'p1', 'p2', 'wants_s4', 's4_nt', 's4_tile', 'NT', 'TW', 'TH', 'KS')


def decision(ks, stride, cin, cout, h, w, b, need, flags, rounds):
    out = (ctypes.c_int * len(FIELDS))()
    pflib.check(pflib.load().pf_debug_conv_decision(ks, stride, cin, cout, h, w, b, need, flags, rounds, out, len(FIELDS)),
                'pf_debug_conv_decision')
    return list(out)


@pytest.fixture
def force():
    L = pflib.load()
    yield lambda *c: pflib.check(L.pf_debug_force_conv(*c), 'pf_debug_force_conv')
    L.pf_debug_force_conv(0, 0, 0, 0)


# ---- s4_resolve: the instantiation launch_conv_s4 runs.  n = nt clamped to [1, ntiles]; 3x3: the first row that matches
def _one_or_two(n):
    return 1 if n == 1 else 2


S4_3X3 = (
    (lambda tile, rounds: tile == 2,                 lambda n: (_one_or_two(n), 32, 16, 1)),
    (lambda tile, rounds: tile == 4 and rounds >= 16, lambda n: (_one_or_two(n), 32, 8, 4)),
    (lambda tile, rounds: tile >= 3 and rounds >= 8,  lambda n: (_one_or_two(n), 32, 8, 2)),
    (lambda tile, rounds: tile >= 3 or tile == 0,     lambda n: (min(n, 4), 32, 8, 1)),
    (lambda tile, rounds: True,                      lambda n: {1: (1, 64, 8, 1), 2: (2, 64, 8, 1)}.get(n, (3, 32, 8, 1))),
)


def expected_shape(ks, nt, tile, ntiles, rounds, kacc):
    n = max(1, min(nt, ntiles))
    if ks == 1:
        return (min(n, 4), 32, 8, 1)
    if kacc:
        return (min(n, 3), 32, 8, 1)
    return next(shape(n) for match, shape in S4_3X3 if match(tile, rounds))


def test_s4_resolve_table(force):
    bad = []
    for nt, tile in itertools.product(range(6), range(5)):
        force(5, nt, tile, 0)   # the forced conv_s4 request reaches s4_resolve as it is
        for ks, ntiles, rounds, kacc in itertools.product((1, 3), range(1, 6), (1, 7, 8, 15, 16, 40), (0, 1)):
            got = decision(ks, 1, 32, 16 * ntiles, 64, 64, 1, 0, SPLIT_PACK | S4_PACK | TUNED | SPLIT_F16 | (KACC if kacc else 0), rounds)
            assert got[5:7] == [nt, tile]
            if tuple(got[7:]) != expected_shape(ks, nt, tile, ntiles, rounds, kacc):
                bad.append((ks, nt, tile, ntiles, rounds, kacc, got[7:]))
    assert not bad, bad[:10]


# ---- decide_conv on every convolution of the default network
def network_convs(h, w):
    """(ks, stride, cin, cout, hout, wout, rounds, flags) of every convolution at an h x w input: rounds of its packed-pair
    weights (conv_s4.hip: s4_rounds), flags = the packings a plan makes for it and whether its input width needs the generic kernel"""
    spec = arch.Spec()
    dims = {spec.input_tensor: (h, w)}
    convs = []
    for o in spec.ops:
        ih, iw = dims[o.srcs[0].tensor]
        if o.kind in (arch.OP_STEM, arch.OP_CONV):
            oh, ow = (ih + 2 * (o.k // 2) - o.k) // o.stride + 1, (iw + 2 * (o.k // 2) - o.k) // o.stride + 1
            per = 2 if o.k == 3 else 8
            entries = sum((s.choff + s.ch + 3) // 4 - s.choff // 4 for s in o.srcs)
            flags = (GENERIC if iw % 4 else 0) | (SPLIT_PACK if o.stride == 1 else 0) | (S4_PACK if o.stride == 1 and o.kind == arch.OP_CONV else 0)
            convs.append((o.k, o.stride, o.cin, o.cout, oh, ow, (entries + per - 1) // per, flags))
        elif o.kind == arch.OP_POOL:
            oh, ow = ih // 2, iw // 2
        elif o.kind == arch.OP_UPSAMPLE:
            oh, ow = dims[o.srcs[1].tensor]
        else:
            oh, ow = ih, iw
        dims[o.dst] = (oh, ow)
    return convs


ON = TUNED | SPLIT_F16
# name -> (h, w, table batch, need, option flags, packings kept, forced choice)
CONFIGS = {'auto B=%d' % b: (1024, 2048, b, 0, ON, ~0, None) for b in (1, 2, 3, 4, 8, 16, 32, 48)}
CONFIGS.update({
    'auto 512x1024 B=16': (512, 1024, 16, 0, ON, ~0, None),
    'auto 800x800 B=8': (800, 800, 8, 0, ON, ~0, None),
    'auto B=16 need=2': (1024, 2048, 16, 2, ON, ~0, None),
    'auto B=16 need=4': (1024, 2048, 16, 4, ON, ~0, None),
    'use_tuned_table off B=16': (1024, 2048, 16, 0, SPLIT_F16, ~0, None),
    'split_f16 off B=16': (1024, 2048, 16, 0, TUNED, ~0, None),
    'no split or S4 packing B=16': (1024, 2048, 16, 0, ON, ~(SPLIT_PACK | S4_PACK), None),
    'force 1,4,2,0': (1024, 2048, 16, 0, ON, ~0, (1, 4, 2, 0)),
    'force 2,1,1,8 need=0': (1024, 2048, 16, 0, ON, ~0, (2, 1, 1, 8)),
    'force 2,1,1,8 need=2': (1024, 2048, 16, 2, ON, ~0, (2, 1, 1, 8)),
    'force 4,2,1,0': (1024, 2048, 16, 0, ON, ~0, (4, 2, 1, 0)),
    'force 5,2,0,0': (1024, 2048, 16, 0, ON, ~0, (5, 2, 0, 0)),
    'force 5,2,4,0': (1024, 2048, 16, 0, ON, ~0, (5, 2, 4, 0)),
})


def decisions(name, force):
    h, w, b, need, opts, keep, forced = CONFIGS[name]
    force(*(forced or (0, 0, 0, 0)))
    return [decision(ks, stride, cin, cout, oh, ow, b, need, (flags & keep) | opts, rounds)
            for ks, stride, cin, cout, oh, ow, rounds, flags in network_convs(h, w)]


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(GOLDEN, 'conv_decision.json')) as f:
        return json.load(f)['decisions']


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_decide_conv_matches_recorded_schedule(name, force, golden):
    got, want = decisions(name, force), golden[name]
    assert len(got) == len(want)
    convs = network_convs(*CONFIGS[name][:2])
    diff = [(convs[i], dict(zip(FIELDS, got[i])), dict(zip(FIELDS, want[i]))) for i in range(len(got)) if got[i] != want[i]]
    assert not diff, diff[:5]


def test_golden_covers_every_kind_and_tile(golden):
    """the recorded cases reach every kernel kind, every conv_s4 tile request and both answers of wants_s4"""
    rows = [r for name in CONFIGS for r in golden[name]]
    assert {r[0] for r in rows} == {0, 1, 2, 4}
    assert {r[6] for r in rows if r[4]} >= {0, 1, 3, 4}
    assert {r[4] for r in rows} == {0, 1}


if __name__ == '__main__':
    L = pflib.load()
    set_force = lambda *c: pflib.check(L.pf_debug_force_conv(*c), 'pf_debug_force_conv')   # noqa: E731
    rec = {'recorded_at': '83472fd + pf_debug_conv_decision over a verbatim copy of the choose lambda and of launch_conv_s4\'s ladder',
           'fields': list(FIELDS), 'decisions': {name: decisions(name, set_force) for name in sorted(CONFIGS)}}
    set_force(0, 0, 0, 0)
    with open(sys.argv[1], 'w') as f:
        json.dump(rec, f, separators=(',', ':'))
        f.write('\n')
