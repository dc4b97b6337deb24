"""The schedule of an inference forward (no GPU): csrc/hardnet_schedule.cpp through pf_debug_hardnet_schedule.  What a GPU run shows only
as profile labels or as a numeric difference is asserted on the step list: which launches fold and which fall back to two launches and
why, which tensors live as packed pairs and that every step reads and writes them as what they are, and the steps of FC-HarDNet-70 at
the timed size.  The numbers of the folded launches are the business of tests/test_gpu_fold_*.py; these tests check the decision."""
import collections
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from panoptic_forecasting_amd import hardnet_arch as arch
from panoptic_forecasting_amd import lib as pflib
from panoptic_forecasting_amd import packing, synth
from test_fold_down_host import both_net, down_net
from test_fold_wide_host import lo_net
from test_gpu_fold_wide import all_forms_net
from test_share_s_host import option  # noqa: F401  (the fixture: process-wide options, the defaults afterwards)

COLS = 30
# columns of a step row (include/pfhip.h: pf_debug_hardnet_schedule)
KIND, OP, CI, NT, TW, TH, KS, CH_KIND = 0, 1, 2, 3, 4, 5, 6, 7
SRC_FMT, DST_FMT, DST_T, POOL, RES, NO_BIAS, DST_NULL, NTILES, NCHUNKS, FOLD_COUT, SHARE_COUT, DOWN_FMT, SB, SE, SRC_T = range(11, 26)
HASH = 29
FOLD_OPTIONS = ('fold_final', 'fold_down', 'fold_lo')


def _enum(name):
    """{enumerator: value} of an enum of csrc/hardnet_schedule.h (the rows carry its numbers)"""
    src = open(os.path.join(ROOT, 'panoptic-forecasting_amd', 'csrc', 'hardnet_schedule.h')).read()
    body = re.search(r'enum %s\b[^{]*\{(.*?)\}' % name, src, re.S).group(1)
    return {n: i for i, n in enumerate(re.findall(r'\w+', body))}


S = _enum('StepKind')
KIND_NAME = {v: k for k, v in S.items()}
FOLDED = (S['S_CONV_S4_TAIL'], S['S_CONV_S4_DOWN'], S['S_CONV_S4_LO'])


def schedule(blob, in_ch, n_cls, b, h, w, out_h=0, out_w=0, stem_t=0, table_batch=0):
    """(formats uint8 [tensors], rows int64 [steps, COLS]) of a forward of the plan the library would create from the blob now"""
    L = pflib.load()
    buf = ctypes.create_string_buffer(blob, len(blob))
    nf, ns = ctypes.c_int(), ctypes.c_int()
    args = (buf, len(blob), in_ch, n_cls, b, h, w, out_h, out_w, stem_t, table_batch)
    pflib.check(L.pf_debug_hardnet_schedule(*args, None, 0, ctypes.byref(nf), None, 0, ctypes.byref(ns)), 'pf_debug_hardnet_schedule')
    fmt = np.zeros(nf.value, dtype=np.uint8)
    rows = np.zeros((ns.value, COLS), dtype=np.int64)
    pflib.check(L.pf_debug_hardnet_schedule(*args, fmt.ctypes.data, fmt.size, ctypes.byref(nf), rows.ctypes.data, ns.value, ctypes.byref(ns)),
                'pf_debug_hardnet_schedule')
    assert nf.value == fmt.size and ns.value == len(rows)
    return fmt, rows


def mini(net, b, h, w):
    """schedule of a (spec, params) test network on a dense input -> (spec, formats, rows)"""
    spec, P = net
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    return (spec,) + schedule(blob, spec.in_ch, spec.n_cls, b, h, w)


@pytest.fixture
def force_conv():
    L = pflib.load()
    yield lambda kind, p0, p1, p2: pflib.check(L.pf_debug_force_conv(kind, p0, p1, p2), 'pf_debug_force_conv')
    L.pf_debug_force_conv(0, 0, 0, 0)


@pytest.fixture
def folds(option):  # noqa: F811
    """folds(mode, **other options): the fold options at `mode` and, as the GPU fold tests run their nets, no pairs and no share / add"""
    def set_(mode, fuse_pairs=0, share_s=0):
        for name in FOLD_OPTIONS:
            option(name, mode, 1)
        option('fuse_pairs', fuse_pairs, 1)
        option('share_s', share_s, 1)
    return set_


@pytest.fixture(scope='module')
def hardnet70():
    with open(os.path.join(GOLDEN, 'calib_seed1234.json')) as f:
        sd = synth.make_state_dict(seed=1234, calib=json.load(f))
    return arch.Spec(36, 11), packing.pack_blob(sd, 36, 11)


def gen():
    return torch.Generator().manual_seed(1)


def steps_of(spec, rows, name):
    """the rows whose first op or whose convolution is the op `name`"""
    i = [op.name for op in spec.ops].index(name)
    return [r for r in rows.tolist() if r[OP] == i or r[CI] == i]


def kinds(rows):
    return collections.Counter(KIND_NAME[k] for k in rows[:, KIND].tolist())


# ---- the fold decisions

def test_down3_and_lo_fold_the_three_tile_producer(folds, force_conv):
    force_conv(5, 3, 0, 0)
    folds(2)
    spec, fmt, rows = mini(down_net(gen(), 16, 46, 96), 2, 16, 40)
    down = [r for r in rows.tolist() if r[KIND] == S['S_CONV_S4_DOWN']]
    assert len(down) == 1 and down[0][NT:KS + 1] == [3, 32, 8, 1] and spec.ops[down[0][OP]].name == 'L4' and down[0][FOLD_COUT] == 96
    assert not steps_of(spec, rows, 'dn') and not steps_of(spec, rows, 'pl')
    assert down[0][DST_NULL] == 0 and 0xFE not in fmt                                   # the slice is stored as ever
    spec, fmt, rows = mini(lo_net(gen(), 16, 46, 63), 2, 32, 80)
    lo = [r for r in rows.tolist() if r[KIND] == S['S_CONV_S4_LO']]
    assert len(lo) == 1 and lo[0][NT:KS + 1] == [3, 32, 8, 1] and spec.ops[lo[0][OP]].name == 'L4' and lo[0][FOLD_COUT] == 63
    out = [t.name for t in spec.tensors].index('out')
    assert lo[0][DST_NULL] == 1 and fmt[out] == 0xFE                                     # `up` is the slice's only reader
    cu = steps_of(spec, rows, 'cu')                                                     # the other half stays as it is
    assert len(cu) == 1 and cu[0][RES] == 1 and cu[0][NO_BIAS] == 0 and cu[0][SB:SE + 1] == [1, 2]
    spec, fmt, rows = mini(lo_net(gen(), 16, 46, 63, second_reader=True), 2, 32, 80)
    lo = [r for r in rows.tolist() if r[KIND] == S['S_CONV_S4_LO']]
    assert len(lo) == 1 and lo[0][DST_NULL] == 0 and fmt[[t.name for t in spec.tensors].index('out')] == 1


def test_down_folds_the_two_tile_producer(folds, force_conv):
    force_conv(5, 2, 0, 0)
    folds(2)
    spec, fmt, rows = mini(down_net(gen(), 10, 28, 64), 2, 16, 40)
    down = [r for r in rows.tolist() if r[KIND] == S['S_CONV_S4_DOWN']]
    assert len(down) == 1 and down[0][NT:KS + 1] == [2, 32, 8, 1] and spec.ops[down[0][OP]].name == 'L4' and not steps_of(spec, rows, 'dn')


def test_both_net_has_one_tail_and_one_down_step(folds, force_conv):
    force_conv(5, 2, 0, 0)
    folds(2)
    spec, fmt, rows = mini(both_net(gen()), 2, 16, 40)
    k = kinds(rows)
    assert k['S_CONV_S4_TAIL'] == 1 and k['S_CONV_S4_DOWN'] == 1 and k['S_CONV_S4_LO'] == 0
    assert [spec.ops[r[OP]].name for r in rows.tolist() if r[KIND] in FOLDED] == ['L4', 'u.L4']
    assert fmt[[t.name for t in spec.tensors].index('u.out')] == 0xFE and not steps_of(spec, rows, 'fin')


def test_all_forms_net_has_one_step_of_each_form(folds, force_conv):
    force_conv(5, 3, 0, 0)
    folds(2)
    spec, fmt, rows = mini(all_forms_net(gen()), 1, 16, 64)
    got = [(KIND_NAME[r[KIND]], spec.ops[r[OP]].name, r[NT]) for r in rows.tolist() if r[KIND] in FOLDED]
    assert got == [('S_CONV_S4_DOWN', 'a.L4', 2), ('S_CONV_S4_DOWN', 'b.L4', 3), ('S_CONV_S4_LO', 'c.L4', 3), ('S_CONV_S4_TAIL', 'd.L4', 2)]
    folds(0)
    _, _, rows0 = mini(all_forms_net(gen()), 1, 16, 64)
    assert len(rows0) == len(rows) + 4 and not any(r[KIND] in FOLDED for r in rows0.tolist())


def _l4(spec, rows):
    st = steps_of(spec, rows, 'L4')
    assert len(st) == 1
    return st[0]


# (net, input size, forced conv, options besides the fold options at `mode`, the mode that must not fold, the field that names the reason)
FALLBACKS = {
    'k_split-down': (lambda: down_net(gen(), 16, 46, 63), (16, 40), (5, 3, 3, 0), {}, 2, lambda s, r: _l4(s, r)[KS] == 2),
    'k_split-lo': (lambda: lo_net(gen(), 16, 46, 63), (32, 80), (5, 3, 3, 0), {}, 2, lambda s, r: _l4(s, r)[KS] == 2),
    'add_launch-down': (lambda: down_net(gen(), 16, 46, 63), (16, 40), (5, 3, 0, 0), {'share_s': 2}, 2,
                        lambda s, r: _l4(s, r)[KIND] == S['S_CONV_S4_ADD']),
    'add_launch-lo': (lambda: lo_net(gen(), 16, 46, 63), (32, 80), (5, 3, 0, 0), {'share_s': 2}, 2,
                      lambda s, r: _l4(s, r)[KIND] == S['S_CONV_S4_ADD']),
    'two_tiles_of_three-down': (lambda: down_net(gen(), 16, 46, 63), (16, 40), (5, 2, 0, 0), {}, 2,
                                lambda s, r: _l4(s, r)[NT] == 2 and _l4(s, r)[NTILES] == 3),
    'two_tiles_of_three-lo': (lambda: lo_net(gen(), 16, 46, 63), (32, 80), (5, 2, 0, 0), {}, 2,
                              lambda s, r: _l4(s, r)[NT] == 2 and _l4(s, r)[NTILES] == 3),
    'dn_of_65_couts': (lambda: down_net(gen(), 10, 28, 65), (16, 40), (5, 2, 0, 0), {}, 2, lambda s, r: steps_of(s, r, 'dn')[0][NTILES] == 5),
    'no_pool': (lambda: down_net(gen(), 10, 28, 64, pool=False), (16, 40), (5, 2, 0, 0), {}, 2, lambda s, r: steps_of(s, r, 'dn')[0][POOL] == 0),
    'rule-down': (lambda: down_net(gen(), 16, 46, 63), (16, 40), (5, 3, 0, 0), {}, 1, lambda s, r: _l4(s, r)[NT] == 3),
    'rule-lo': (lambda: lo_net(gen(), 16, 46, 63), (32, 80), (5, 3, 0, 0), {}, 1, lambda s, r: _l4(s, r)[NT] == 3),
    'rule-down-two_tiles': (lambda: down_net(gen(), 10, 28, 64), (16, 40), (5, 2, 0, 0), {}, 1, lambda s, r: _l4(s, r)[NT] == 2),
}


@pytest.mark.parametrize('case', sorted(FALLBACKS))
def test_fallbacks_give_the_step_list_of_the_option_at_0(case, folds, force_conv):
    """what keeps a fold from happening - a K split, L4 being the add launch of a share pair, three cout tiles in workgroups of two, a
    reader of 65 couts, no pool, the rule at sizes nobody measured -: every row, hashes included, and every format as with the options
    at 0, and the field that names the reason holds"""
    net, (h, w), forced, other, mode, reason = FALLBACKS[case]
    force_conv(*forced)
    got = {}
    for m in (0, mode):
        folds(m, **other)
        got[m] = mini(net(), 2, h, w)
    spec, fmt0, rows0 = got[0]
    _, fmt, rows = got[mode]
    assert not any(r[KIND] in FOLDED for r in rows.tolist())
    assert np.array_equal(rows, rows0) and np.array_equal(fmt, fmt0)
    assert reason(spec, rows)


# ---- the formats

def check_formats(spec, fmt, rows):
    """every step reads and writes each tensor as what the format table says it is.  A tensor whose last slice is elided (0xFE) holds
    packed pairs in its other slices, which the block's own layers read; read here: as the convolution's ranges name it"""
    fmt = fmt.tolist()
    packed = lambda t: fmt[t] in (1, 0xFE)  # noqa: E731
    elided = {}                                                  # tensor -> (step, first channel, channels) of the slice never stored
    for k, r in enumerate(rows.tolist()):
        if r[KIND] == S['S_CONV_S4_TAIL'] or (r[KIND] == S['S_CONV_S4_LO'] and r[DST_NULL]):
            L = spec.ops[r[OP]]
            assert L.dst not in elided
            elided[L.dst] = (k, L.dst_choff, L.cout)
    assert sorted(elided) == [t for t, f in enumerate(fmt) if f == 0xFE]
    n_conv = 0
    for k, r in enumerate(rows.tolist()):
        op = spec.ops[r[OP]]
        if r[CI] < 0:                                            # stem, front end, pool, upsample, head, range check
            reads = [(s.tensor, 0, spec.tensors[s.tensor].channels) for s in op.srcs[:1]]
            if r[KIND] == S['S_STEM_FRONT']:
                assert r[DST_FMT] == int(packed(r[DST_T])) and fmt[op.dst] == 1 and fmt[spec.ops[r[OP] + 1].dst] == 0xFF
            elif r[KIND] != S['S_RANGE_CHECK']:
                assert fmt[r[DST_T]] == 0 and r[DST_FMT] == 0, (k, r)
                assert all(fmt[t] == 0 for t, _, _ in reads), (k, r)
        else:
            n_conv += 1
            conv = spec.ops[r[CI]]
            reads = [(r[SRC_T + j], conv.srcs[j].choff, conv.srcs[j].ch) for j in range(r[SB], r[SE])]
            assert reads and all(t >= 0 for t, _, _ in reads)
            assert (r[SRC_FMT] == 1) == all(packed(t) for t, _, _ in reads), (k, r)
            assert (r[DST_FMT] == 1) == packed(r[DST_T]), (k, r)
            if r[KIND] == S['S_CONV_S4_DOWN']:                   # ... and the pooled tensor of the folded 1x1 conv
                assert r[DOWN_FMT] == int(packed(spec.ops[r[OP] + 2].dst)), (k, r)
        for t, c0, n in reads:
            assert fmt[t] != 0xFF, (k, r)
            if t in elided:                                      # nobody reads the slice that does not exist
                _, e0, en = elided[t]
                assert c0 + n <= e0 or c0 >= e0 + en, (k, r)
    assert n_conv > 0


MINI = {'down': (lambda: down_net(gen(), 16, 46, 96), 16, 40), 'lo': (lambda: lo_net(gen(), 16, 46, 63), 32, 80),
        'lo-second_reader': (lambda: lo_net(gen(), 16, 46, 63, second_reader=True), 32, 80), 'both': (lambda: both_net(gen()), 16, 40),
        'all_forms': (lambda: all_forms_net(gen()), 16, 64), 'all_forms-odd_width': (lambda: all_forms_net(gen()), 16, 66)}


@pytest.mark.parametrize('mode', [0, 2])
@pytest.mark.parametrize('net', sorted(MINI))
def test_formats_of_the_mini_nets(net, mode, folds, force_conv):
    force_conv(5, 3, 0, 0)
    make, h, w = MINI[net]
    for pairs, share in ((0, 0), (1, 1), (2, 2)):
        folds(mode, fuse_pairs=pairs, share_s=share)
        spec, fmt, rows = mini(make(), 2, h, w)
        check_formats(spec, fmt, rows)
        assert (1 in fmt) == (w % 4 == 0)


@pytest.mark.parametrize('b,h,w,stem_t', [(2, 64, 128, 3), (2, 64, 128, 0), (4, 1024, 2048, 3), (4, 1024, 2048, 0)])
def test_formats_of_fchardnet70(b, h, w, stem_t, hardnet70):
    spec, blob = hardnet70
    fmt, rows = schedule(blob, 36, 11, b, h, w, h, w, stem_t)
    check_formats(spec, fmt, rows)
    assert 1 in fmt or (h, stem_t) == (64, 0)      # (at 64 x 128 the fp32-source kernels are chosen throughout; the front end packs anyway)


# ---- FC-HarDNet-70 at the timed size, through the fused stem

# Per-kind step counts, default options.  Taken from a dump of the schedule as it was before build_schedule was split into passes (the
# same debug entry over the untouched function: profiles/hardnet_schedule_split.md), not from the code under test
TIMED_COUNTS = {
    4: {'S_CONV_S4': 49, 'S_CONV_S4_DOWN': 2, 'S_CONV_S4_LO': 1, 'S_CONV_S4_TAIL': 1, 'S_CONV_WAVE': 10, 'S_HEAD': 1, 'S_PAIR': 2, 'S_STEM_FRONT': 1},
    16: {'S_CONV_S4': 63, 'S_CONV_S4_DOWN': 2, 'S_CONV_S4_LO': 1, 'S_CONV_S4_TAIL': 1, 'S_HEAD': 1, 'S_STEM_FRONT': 1},
    32: {'S_CONV_S4': 59, 'S_CONV_S4_ADD': 2, 'S_CONV_S4_DOWN': 2, 'S_CONV_S4_LO': 1, 'S_CONV_S4_SHARE': 2, 'S_CONV_S4_TAIL': 1, 'S_HEAD': 1,
         'S_STEM_FRONT': 1},
}


@pytest.mark.parametrize('b', [4, 16, 32])
def test_timed_configuration_folds_the_two_128x256_transitions(b, hardnet70):
    spec, blob = hardnet70
    fmt, rows = schedule(blob, 36, 11, b, 1024, 2048, 1024, 2048, 3)
    assert dict(kinds(rows)) == TIMED_COUNTS[b]
    assert rows[0, KIND] == S['S_STEM_FRONT'] and rows[-1, KIND] == S['S_HEAD']
    wide = [(KIND_NAME[r[KIND]], spec.ops[r[OP]].name, spec.ops[r[OP] + (2 if r[KIND] == S['S_CONV_S4_LO'] else 1)].name)
            for r in rows.tolist() if r[KIND] in FOLDED and r[NT] == 3]
    assert wide == [('S_CONV_S4_DOWN', 'base.7.layers.3', 'base.8'), ('S_CONV_S4_LO', 'denseBlocksUp.2.layers.3', 'conv1x1_up.3')]
    assert all(r[NT:KS + 1] == [r[NT], 32, 8, 1] and r[NT] in (2, 3) for r in rows.tolist() if r[KIND] in FOLDED)


def test_table_batch_16_at_batch_4_chooses_as_batch_16(hardnet70):
    spec, blob = hardnet70
    _, at16 = schedule(blob, 36, 11, 16, 1024, 2048, 1024, 2048, 3)
    _, as16 = schedule(blob, 36, 11, 4, 1024, 2048, 1024, 2048, 3, table_batch=16)
    _, at4 = schedule(blob, 36, 11, 4, 1024, 2048, 1024, 2048, 3)
    assert np.array_equal(as16[:, :CH_KIND + 4], at16[:, :CH_KIND + 4])          # kinds, ops, conv_s4 shapes, the other kernels' choices
    assert not np.array_equal(as16[:, HASH], at16[:, HASH])                      # (the arguments are those of four frames)
    assert len(at4) != len(at16)


def test_two_calls_give_identical_rows(hardnet70, folds, force_conv):
    spec, blob = hardnet70
    for stem_t in (3, 0):
        a, b = schedule(blob, 36, 11, 4, 256, 512, 256, 512, stem_t), schedule(blob, 36, 11, 4, 256, 512, 256, 512, stem_t)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(set(a[1][:, HASH].tolist())) > len(a[1]) // 2
    force_conv(5, 3, 0, 0)
    folds(2)
    a, b = mini(all_forms_net(gen()), 1, 16, 64), mini(all_forms_net(gen()), 1, 16, 64)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
