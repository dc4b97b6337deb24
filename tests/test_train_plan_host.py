"""The plan of a bg training step (no GPU): the workspace layout of csrc/train_layout.cpp and the schedule of csrc/train_schedule.cpp
through pf_debug_train_plan.  What a GPU run shows only as a numeric difference or a race is asserted on the tables: regions that do
not overlap, every gradient channel initialised exactly once and before anything is added to it, reads after the last write, and the
forks / waits / dones of the dy slots in the order the side streams need."""
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from helpers import mini_net, plan_path_stats, train_plan_tables
from panoptic_forecasting_amd import hardnet_arch as arch
from panoptic_forecasting_amd import lib as pflib
from panoptic_forecasting_amd import packing, synth

STORE, ADD, CLEAR, READ = range(4)


def _enum(name):
    """{enumerator: value} of an enum of csrc/train_plan.h (the tables carry its numbers)"""
    src = open(os.path.join(ROOT, 'panoptic-forecasting_amd', 'csrc', 'train_plan.h')).read()
    body = re.search(r'enum %s\b[^{]*\{(.*?)\}' % name, src, re.S).group(1)
    return {n: i for i, n in enumerate(re.findall(r'\w+', body))}


T, R = _enum('TStepKind'), _enum('TRegionKind')


@pytest.fixture(scope='module')
def nets():
    """{name: (spec, blob)}: the mini net of the GPU training tests and the FC-HarDNet-70 table as test_share_s_host.py builds it"""
    import torch
    sp = mini_net()
    dummy = {op.name: (torch.zeros(op.cout, op.cin, op.k, op.k), torch.zeros(op.cout)) for op in sp.conv_ops()}
    with open(os.path.join(GOLDEN, 'calib_seed1234.json')) as f:
        sd = synth.make_state_dict(seed=1234, calib=json.load(f))
    return {'mini': (sp, packing.pack_blob(None, sp.in_ch, sp.n_cls, spec=sp, params=dummy)),
            'hardnet70': (arch.Spec(36, 11), packing.pack_blob(sd, 36, 11))}


@pytest.fixture
def option():
    """process-wide options for the plans a test asks for; the library's defaults afterwards"""
    L = pflib.load()
    touched = {}

    def set_(name, value, default):
        touched[name] = default
        pflib.check(L.pf_set_option(name.encode(), value), 'pf_set_option')
    yield set_
    for name, default in touched.items():
        pflib.check(L.pf_set_option(name.encode(), default), 'pf_set_option')


# (net, B, H, W, out_h, out_w): the mini net with a pooled level of width 10 and with widths 35 / 17, all odd; FC-HarDNet-70 small
# and at the timed configuration, whose 50- and 25-pixel levels are odd
CASES = {'mini-24x40': ('mini', 3, 24, 40, 45, 81), 'mini-34x70': ('mini', 3, 34, 70, 65, 141),
         'hardnet70-64x128': ('hardnet70', 2, 64, 128, 64, 128), 'hardnet70-800x800': ('hardnet70', 8, 800, 800, 800, 800)}


def _dims(spec, h, w):
    """(h, w) per tensor (None: never produced): csrc/pf_net.cpp, propagate_dims"""
    d = [None] * len(spec.tensors)
    d[spec.ops[0].srcs[0].tensor] = (h, w)
    for op in spec.ops:
        ih, iw = d[op.srcs[0].tensor]
        if op.kind in (arch.OP_STEM, arch.OP_CONV):
            pad = op.k // 2
            out = ((ih + 2 * pad - op.k) // op.stride + 1, (iw + 2 * pad - op.k) // op.stride + 1)
        elif op.kind == arch.OP_POOL:
            out = (ih // 2, iw // 2)
        elif op.kind == arch.OP_UPSAMPLE:
            out = d[op.srcs[1].tensor]
        else:
            continue
        d[op.dst] = out
    return d


@pytest.fixture(params=[(side, s4) for side in (0, 1) for s4 in (0, 1)], ids=lambda p: 'side%d-s4%d' % p)
def plan(request, nets, option):
    """plan(case) -> (spec, case tuple, regions, step rows, range rows per step, dy slots, side streams, (side, s4))"""
    side, s4 = request.param
    option('train_side_stream', side, 1)
    option('train_forward_s4', s4, 0)

    def get(case):
        net, b, h, w, oh, ow = CASES[case]
        spec, blob = nets[net]
        regions, rows, (slots, streams) = train_plan_tables(blob, spec.in_ch, spec.n_cls, b, h, w, oh, ow)
        assert rows[0][0] == 0 and set(rows[:, 0]) == {0, 1}
        steps, ranges = [], []
        for r in rows.tolist():
            if r[0] == 0:
                steps.append(r[1:])
                ranges.append([])
            else:
                ranges[-1].append(r[1:])
        return spec, CASES[case], regions, steps, ranges, slots, streams, (side, s4)
    return get


@pytest.mark.parametrize('case', sorted(CASES))
def test_regions_are_aligned_disjoint_and_hold_their_tensors(case, plan):
    spec, (_, b, h, w, oh, ow), regions, _, _, slots, _, (side, s4) = plan(case)
    assert regions[-1].tolist()[:3] == [R['R_TOTAL'], 0, 0] and R['R_TOTAL'] not in regions[:-1, 0]
    total, reg = int(regions[-1, 3]), regions[:-1]
    assert (reg[:, 2] % 256 == 0).all()
    reg = reg[np.argsort(reg[:, 2], kind='stable')]
    ends = reg[:, 2] + reg[:, 3]
    assert (reg[:, 3] >= 0).all() and (ends[:-1] <= reg[1:, 2]).all() and ends[-1] <= total
    d = _dims(spec, h, w)
    held = {(int(k), int(i)): int(n) for k, i, _, n in reg}
    assert len(held) == len(reg)                            # no region is handed out twice
    inp = spec.ops[0].srcs[0].tensor
    for t, ten in enumerate(spec.tensors):
        for kind in ('R_ACT', 'R_GRAD'):
            want = d[t] is not None and not (kind == 'R_GRAD' and t == inp)
            assert ((R[kind], t) in held) == want, (kind, ten.name)
            if want:
                assert held[(R[kind], t)] >= b * ten.channels * d[t][0] * d[t][1] * 4, (kind, ten.name)
    assert sum(k == R['R_DY'] for k, _ in held) == (slots if side else 1)
    assert any(k == R['R_S4ACT'] for k, _ in held) == bool(s4)
    assert not any(k == R['R_TUNE_GRAD'] for k, _ in held)


@pytest.mark.parametrize('case', sorted(CASES))
def test_every_gradient_channel_is_initialised_once_then_added_to_then_read(case, plan):
    spec, (_, b, h, w, oh, ow), regions, steps, ranges, _, _, _ = plan(case)
    has_grad = sorted(int(i) for k, i in regions[:, :2] if k == R['R_GRAD'])
    log = {t: [[] for _ in range(spec.tensors[t].channels)] for t in has_grad}     # per channel: its accesses in step order
    for i, rs in enumerate(ranges):
        for t, c0, n, access in rs:
            assert t in log and 0 <= c0 and n > 0 and c0 + n <= spec.tensors[t].channels, (i, t, c0, n)
            for c in range(c0, c0 + n):
                log[t][c].append(access)
    n_read = 0
    for t in has_grad:
        for c, acc in enumerate(log[t]):
            where = (spec.tensors[t].name, c, acc)
            assert acc and acc[0] in (STORE, CLEAR), where                         # no channel is left uninitialised, none is added to first
            assert sum(a in (STORE, CLEAR) for a in acc) == 1, where
            writes = [i for i, a in enumerate(acc) if a != READ]
            reads = [i for i, a in enumerate(acc) if a == READ]
            assert not reads or reads[0] > writes[-1], where
            n_read += len(reads)
    assert n_read > 0
    # the steps that write and read gradients are the ones the rows come from
    kinds_with_rows = {steps[i][0] for i, rs in enumerate(ranges) if rs}
    assert {T['T_BN_BWD'], T['T_BIAS_BWD'], T['T_UPSAMPLE_BWD'], T['T_POOL_BWD']} <= kinds_with_rows      # (FC-HarDNet-70 needs no clear)
    assert kinds_with_rows & {T['T_CONV_DMA'], T['T_UNPAD'], T['T_UNPAD_MULTI']}
    for i, st in enumerate(steps):
        if st[0] in (T['T_BN_BWD'], T['T_BIAS_BWD'], T['T_POOL_BWD'], T['T_ZERO_CHANNELS']):
            assert ranges[i], (i, st)


@pytest.mark.parametrize('case', sorted(CASES))
def test_side_stream_steps_fork_wait_and_finish_in_slot_order(case, plan):
    spec, _, _, steps, _, slots, streams, (side, _) = plan(case)
    kind = [s[0] for s in steps]
    n_conv = len(spec.conv_ops())
    at = {name: [i for i, k in enumerate(kind) if k == T[name]] for name in ('T_FORK', 'T_WAIT_WG', 'T_WG_DONE', 'T_WGRAD')}
    dy = [i for i, k in enumerate(kind) if k in (T['T_BN_BWD'], T['T_BIAS_BWD'])]      # the steps that fill a dy slot
    assert len(at['T_WGRAD']) == len(dy) == n_conv
    if not side:
        assert not at['T_FORK'] and not at['T_WAIT_WG'] and not at['T_WG_DONE']
        assert all(s[1] == -1 for s in steps)
        return
    assert len(at['T_FORK']) == len(at['T_WG_DONE']) == n_conv and len(at['T_WAIT_WG']) == max(0, n_conv - slots)
    assert all(steps[i][1] == -1 for i in range(len(steps)) if kind[i] not in (T['T_FORK'], T['T_WGRAD'], T['T_WG_DONE']))
    for n in range(n_conv):
        fork, wg, done = at['T_FORK'][n], at['T_WGRAD'][n], at['T_WG_DONE'][n]
        assert dy[n] < fork < wg < done and (n + 1 == n_conv or done < dy[n + 1])
        assert steps[wg][1] == n % streams
        assert steps[fork][1:3] == [n % streams, n % slots] and steps[done][1:3] == [n % streams, n % slots]
        if n >= slots:      # the slot is refilled: after a wait for the weight gradient that last read it
            wait = at['T_WAIT_WG'][n - slots]
            assert steps[wait][2] == n % slots and at['T_WG_DONE'][n - slots] < wait < dy[n]


def test_path_statistics_of_the_timed_configuration(plan):
    spec, _, _, steps, ranges, _, _, (side, s4) = plan('hardnet70-800x800')
    rows = np.array([[0] + s for s in steps], dtype=np.int32)
    stats = plan_path_stats(rows)
    assert stats[0] > 0 and stats[6] == 0 and all(stats[k] > 0 for k in (3, 4, 5)), stats
    assert (stats[7] >= 60) if s4 else stats[7] == 0, stats
