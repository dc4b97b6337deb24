"""The schedule of an fg forward (no GPU): every launch of csrc/fg_schedule.cpp with its buffers, and the workspace layout, through
pf_debug_fg_schedule - for every (T_in, T_out) the ABI allows, both arithmetics and two batch sizes.  What a GPU run shows only as a
numeric difference, and only at the few lengths the GPU tests run, is asserted on the tables: the h0 ring, the h1 ping-pong and the
in-place c never hand a launch a buffer it also writes, every read finds what an earlier launch wrote, and each ConvLSTM cell reads the
h its predecessor wrote."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from panoptic_forecasting_amd import lib as pflib

HEADER = open(os.path.join(ROOT, 'panoptic-forecasting_amd', 'csrc', 'fg_net.h')).read()


def _enum(pattern):
    """{enumerator: value} of an enum of csrc/fg_net.h (the tables carry its numbers)"""
    return {n: i for i, n in enumerate(re.findall(r'\w+', re.search(pattern, HEADER, re.S).group(1)))}


R, K = _enum(r'enum Region \{(.*?)\}'), _enum(r'enum StepKind \{(.*?)\}')
G, EPI = _enum(r'enum \{ (G_ME0.*?)\}'), {'lstm': 0, 'relu': 1, 'bias': 2, 'deconv': 3}
FG_SLOT0 = int(re.search(r'FG_SLOT0 = (\d+)', HEADER).group(1))
PAIR, STATUS_BYTES = 1, 1024                                    # include/pfhip.h: PF_FG_PAIR, PF_FG_STATUS_BYTES
C, HW, IFH, TF, HID = 256, 196, 64, 16, 128
PAIR_GEMMS = ['G_ME0', 'G_ME1', 'G_MD0', 'G_MD1', 'G_F1', 'G_F2', 'G_F3', 'G_F4']      # the eight 3x3 GEMMs, in pack order
CTOT = dict(G_ME0=528, G_ME1=512, G_MD0=528, G_MD1=512, G_MEO=256, G_MDO=256, G_F1=256, G_F2=256, G_F3=256, G_F4=256, G_DC=256)
OPS = ('vec', 'x', 'h', 'out', 'c')
WS = range(R['R_STATUS'], R['R_FEATS'])                        # the workspace regions


def tables(n, t_in, t_out, flags):
    """(regions [r][3], steps: list of dicts, labels) of pf_debug_fg_schedule - include/pfhip.h documents the rows"""
    L = pflib.load()
    nr, ns = ctypes.c_int(), ctypes.c_int()
    pflib.check(L.pf_debug_fg_schedule(n, t_in, t_out, flags, None, 0, ctypes.byref(nr), None, None, 0, ctypes.byref(ns)), 'pf_debug_fg_schedule')
    regions, rows = np.zeros((nr.value, 3), dtype=np.int64), np.zeros((ns.value, 30), dtype=np.int64)
    labels = ctypes.create_string_buffer(64 * ns.value)
    pflib.check(L.pf_debug_fg_schedule(n, t_in, t_out, flags, regions.ctypes.data, nr.value, ctypes.byref(nr), rows.ctypes.data, labels,
                                       ns.value, ctypes.byref(ns)), 'pf_debug_fg_schedule')
    assert (nr.value, ns.value) == (len(regions), len(rows))
    steps = []
    for r in rows.tolist():
        st = dict(zip(('kind', 'gemm', 'epi', 'nvec', 'nx', 'nh', 'ctot', 'pair', 'slot', 't'), r[:10]))
        for k, name in enumerate(OPS):      # (region, offset, stride, span); None = the launch has no such operand
            st[name] = tuple(r[10 + 4 * k:14 + 4 * k]) if r[10 + 4 * k] else None
        steps.append(st)
    return regions, steps, [labels.raw[64 * i:64 * i + 64].split(b'\0')[0].decode() for i in range(ns.value)]


CASES = [(n, ti, to, fl) for n in (1, 5) for ti in range(1, 17) for to in range(1, 17) for fl in (0, PAIR)]


@pytest.fixture(scope='module')
def all_tables():
    return {case: tables(*case) for case in CASES}


def intervals(op, n):
    """the floats of its region an operand covers over n instances: [(begin, end)], merged where instances are contiguous"""
    _, off, stride, span = op
    if stride == span:
        return [(off, off + n * span)]
    return [(off + i * stride, off + i * stride + span) for i in range(n)]


def overlap(a, b):
    return any(x0 < y1 and y0 < x1 for x0, x1 in a for y0, y1 in b)


def add(written, new):
    out = []
    for a, b in sorted(written + new):
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def expected_sequence(t_in, t_out, pair):
    """(kind, label, GEMM id) of every launch, in the order pf_fg_forward has always enqueued them"""
    def conv3(epi, name, g):
        return (K['K_PAIR'], 'pf::fg::pair_kernel<%s> %s' % (epi, name), G[g]) if pair else \
            (K['K_GEMM'], 'pf::fg::gemm_kernel<9,%s> %s' % (epi, name), G[g])
    inst = (K['K_INST_FEAT'], 'pf::fg::inst_feat_kernel', -1)
    out = lambda g: (K['K_GEMM'], 'pf::fg::gemm_kernel<1,bias> out', G[g])
    seq = [(K['K_STATUS'], '', -1)] if pair else []
    seq += [inst, (K['K_TRAJ_ENC'], 'pf::fg::traj_encoder_kernel', -1)]
    seq += [conv3('lstm', 'enc0', 'G_ME0')] * t_in + [conv3('lstm', 'enc1', 'G_ME1')] * t_in + [out('G_MEO')]
    for _ in range(t_out):
        seq += [inst, (K['K_TRAJ_DEC'], 'pf::fg::traj_decoder_kernel', -1), conv3('lstm', 'dec0', 'G_MD0'), conv3('lstm', 'dec1', 'G_MD1'),
                out('G_MDO')]
    seq += [(K['K_GATHER'], '', -1)] + [conv3('relu', 'mask_fcn', 'G_F%d' % i) for i in (1, 2, 3, 4)]
    return seq + [(K['K_GEMM'], 'pf::fg::gemm_kernel<1,deconv>', G['G_DC']), (K['K_PREDICT'], 'pf::fg::predictor_kernel', -1)]


def test_step_count_kinds_and_labels_in_launch_order(all_tables):
    for (n, t_in, t_out, flags), (_, steps, labels) in all_tables.items():
        assert len(steps) == 3 + 2 * t_in + 5 * t_out + 7 + (1 if flags else 0)
        assert [(st['kind'], la, st['gemm']) for st, la in zip(steps, labels)] == expected_sequence(t_in, t_out, flags == PAIR)
        gemms = [st for st in steps if st['gemm'] >= 0]
        assert [st['epi'] for st in gemms] == [EPI['lstm']] * (2 * t_in) + [EPI['bias']] + [EPI['lstm'], EPI['lstm'], EPI['bias']] * t_out + \
            [EPI['relu']] * 4 + [EPI['deconv']]
        # the decoder's launches carry their step, the encoder's -1
        assert [st['t'] for st in steps if st['kind'] in (K['K_INST_FEAT'], K['K_TRAJ_ENC'], K['K_TRAJ_DEC'])] == \
            [-1, -1] + [t for t in range(t_out) for _ in range(2)]


def test_workspace_regions_are_aligned_disjoint_and_end_at_the_reported_size(all_tables):
    L = pflib.load()
    for (n, t_in, t_out, flags), (regions, _, _) in all_tables.items():
        need = ctypes.c_size_t()
        if flags:
            pflib.check(L.pf_fg_pair_workspace(n, t_in, t_out, ctypes.byref(need)), 'pf_fg_pair_workspace')
        else:
            pflib.check(L.pf_fg_workspace(n, t_in, t_out, 0, ctypes.byref(need)), 'pf_fg_workspace')
        assert regions[-1].tolist() == [R['R_NONE'], 0, need.value]
        reg = regions[:-1]
        assert reg[:, 0].tolist() == list(WS)                                   # each once, in layout order
        assert (reg[:, 1] % 256 == 0).all() and (reg[:, 2] >= 0).all()
        ends = reg[:, 1] + reg[:, 2]
        assert (ends[:-1] <= reg[1:, 1]).all()
        assert -(-int(ends[-1]) // 256) * 256 == need.value                     # nothing behind the last region but its padding
        # the pair workspace = the status block in front of the flags = 0 workspace
        plain = all_tables[(n, t_in, t_out, 0)][0]
        assert reg[0].tolist() == [R['R_STATUS'], 0, STATUS_BYTES if flags else 0]
        assert (reg[1:, 1] == plain[1:-1, 1] + (STATUS_BYTES if flags else 0)).all() and (reg[1:, 2] == plain[1:-1, 2]).all()
        assert need.value == plain[-1, 2] + (STATUS_BYTES if flags else 0)
        p = n * C * HW
        want = dict(R_INSTF=n * t_in * IFH, R_INSTD=n * IFH, R_GRUH=n * HID, R_TFE=n * t_in * TF, R_TFD=n * TF, R_H0=max(t_in, 2) * p,
                    R_C0=p, R_H1=2 * p, R_C1=p, R_YA=p, R_YB=p, R_YD=n * C * 784)
        assert {int(r): int(b) for r, _, b in reg[1:]} == {R[k]: 4 * v for k, v in want.items()}


def region_floats(regions, n, t_in, t_out):
    size = {int(r): int(b) // 4 for r, _, b in regions[:-1]}
    p = n * C * HW
    size.update({R['R_FEATS']: t_in * p, R['R_MASK_FEATS']: (1 + t_out) * p, R['R_OUTPUT_FEATS']: p, R['R_MASKS']: n * 784})
    return size


def test_operands_stay_inside_their_regions_and_out_aliases_no_input(all_tables):
    for (n, t_in, t_out, flags), (regions, steps, _) in all_tables.items():
        size = region_floats(regions, n, t_in, t_out)
        for st in steps:
            for name in OPS:
                if st[name]:
                    region, off, stride, span = st[name]
                    assert region != R['R_STATUS'] and span > 0 and stride >= span and off >= 0, (st, name)
                    assert off + (n - 1) * stride + span <= size[region], (st, name)
            for name in ('vec', 'x', 'h'):
                a, b = st[name], st['out']
                if a and b and a[0] == b[0]:
                    assert not overlap(intervals(a, n), intervals(b, n)), (st, name)
            if st['c']:                 # the one in-place operand: a region of its own, never another operand's
                assert all(not st[name] or st[name][0] != st['c'][0] for name in ('vec', 'x', 'h', 'out')), st


def test_every_read_was_written_by_an_earlier_step(all_tables):
    tracked = set(WS) | {R['R_MASK_FEATS'], R['R_OUTPUT_FEATS']}              # feats alone comes from the caller
    for (n, t_in, t_out, flags), (_, steps, _) in all_tables.items():
        written = {r: [] for r in tracked}
        for st in steps:
            reads = [st[name] for name in ('vec', 'x', 'h') if st[name]]
            # the cell state is read when the cell has an h (c = 0 goes with h = 0); the decoder's GRU continues the encoder's state
            if st['c'] and (st['h'] or st['kind'] == K['K_TRAJ_DEC']):
                reads.append(st['c'])
            for op in reads:
                if op[0] in tracked:
                    for a, b in intervals(op, n):
                        assert any(x0 <= a and b <= x1 for x0, x1 in written[op[0]]), (st, op)
            for op in (st['out'], st['c']):
                if op and op[0] in tracked:
                    written[op[0]] = add(written[op[0]], intervals(op, n))
        # all of mask_feats and output_feats is written by the end
        p = n * C * HW
        assert written[R['R_MASK_FEATS']] == [(0, (1 + t_out) * p)] and written[R['R_OUTPUT_FEATS']] == [(0, p)]


def test_convlstm_cells_chain_through_h_and_c(all_tables):
    for (n, t_in, t_out, flags), (_, steps, _) in all_tables.items():
        layer = [[st for st in steps if st['gemm'] in (G[a], G[b])] for a, b in (('G_ME0', 'G_MD0'), ('G_ME1', 'G_MD1'))]
        assert [len(l) for l in layer] == [t_in + t_out] * 2
        for l, cells in enumerate(layer):
            assert cells[0]['h'] is None and all(c['h'] for c in cells[1:])
            assert all(c['h'] == prev['out'] for prev, c in zip(cells, cells[1:]))               # the range the previous cell wrote
            assert len({c['c'] for c in cells}) == 1 and cells[0]['c'][0] == R['R_C%d' % l]
            assert all(c['out'][0] == R['R_H%d' % l] and c['out'][3] == C * HW and c['nh'] == C for c in cells)
        assert all(c1['x'] == c0['out'] for c0, c1 in zip(*layer))                                # layer 1 at step t reads layer 0's h of step t
        # layer 0's inputs: feats[:, t] with the encoder's traj_feat_out of step t, then mask_feats[:, t] with the decoder's
        for t, c in enumerate(layer[0]):
            if t < t_in:
                assert c['x'] == (R['R_FEATS'], t * C * HW, t_in * C * HW, C * HW) and c['vec'] == (R['R_TFE'], t * TF, t_in * TF, TF)
            else:
                assert c['x'] == (R['R_MASK_FEATS'], (t - t_in) * C * HW, (1 + t_out) * C * HW, C * HW) and c['vec'] == (R['R_TFD'], 0, TF, TF)
        # the 1x1 output convs read layer 1's newest h and fill mask_feats slot by slot
        outs = [st for st in steps if st['gemm'] in (G['G_MEO'], G['G_MDO'])]
        assert [o['x'] for o in outs] == [layer[1][t_in - 1 + k]['out'] for k in range(1 + t_out)]
        assert [o['out'] for o in outs] == [(R['R_MASK_FEATS'], k * C * HW, (1 + t_out) * C * HW, C * HW) for k in range(1 + t_out)]


def test_k_sources_match_the_packed_weights_and_pair_steps_own_their_slots(all_tables):
    names = {v: k for k, v in G.items()}
    for (n, t_in, t_out, flags), (_, steps, _) in all_tables.items():
        for st in steps:
            if st['gemm'] >= 0:
                assert st['nvec'] + st['nx'] + st['nh'] == st['ctot'] == CTOT[names[st['gemm']]], st
                assert (st['nvec'] > 0) == (st['vec'] is not None) and st['x'] and st['nx'] == C
        pairs = [st for st in steps if st['kind'] == K['K_PAIR']]
        three = [st for st in steps if st['gemm'] >= 0 and names[st['gemm']] in PAIR_GEMMS]
        if not flags:
            assert not pairs and all(st['pair'] == st['slot'] == -1 for st in steps) and K['K_STATUS'] not in [st['kind'] for st in steps]
            continue
        assert steps[0]['kind'] == K['K_STATUS'] and pairs == three                              # every 3x3 GEMM and nothing else
        assert {names[st['gemm']] for st in pairs} == set(PAIR_GEMMS)
        assert all(st['nvec'] % 8 == 0 and st['nx'] % 8 == 0 and st['nh'] % 8 == 0 for st in pairs)
        assert all(st['pair'] == PAIR_GEMMS.index(names[st['gemm']]) for st in pairs)
        assert [st['slot'] for st in pairs] == list(range(len(pairs))) and len(pairs) == 2 * (t_in + t_out) + 4
        assert all(st['pair'] == st['slot'] == -1 for st in steps if st['kind'] != K['K_PAIR'])
        assert FG_SLOT0 + 3 * len(pairs) <= STATUS_BYTES // 4
    assert len([st for st in all_tables[(5, 16, 16, PAIR)][1] if st['kind'] == K['K_PAIR']]) == 68


def test_refusals_carry_the_codes_of_pf_fg_forward():
    L = pflib.load()
    nr, ns = ctypes.c_int(), ctypes.c_int()
    for n, t_in, t_out, flags, code, text in [(-1, 3, 3, 0, -1, b'bad dims'), ((1 << 20) + 1, 3, 3, 0, -1, b'bad dims'), (4, 0, 3, 0, -1, b'bad dims'),
                                              (4, 17, 3, 1, -1, b'bad dims'), (4, 3, 0, 0, -1, b'bad dims'), (4, 3, 17, 1, -1, b'bad dims'),
                                              (4, 3, 3, 2, -5, b'unsupported flags'), (4, 3, 3, 3, -5, b'unsupported flags'),
                                              (4, 0, 3, 4, -5, b'unsupported flags')]:
        assert L.pf_debug_fg_schedule(n, t_in, t_out, flags, None, 0, ctypes.byref(nr), None, None, 0, ctypes.byref(ns)) == code
        assert text in L.pf_last_error()
        # the same answer as the forward gives before it touches a buffer
        assert L.pf_fg_forward(None, flags, n, t_in, t_out, 64, *([None] * 14), None, 0, None) == code
        assert text in L.pf_last_error()
    assert L.pf_debug_fg_schedule(4, 3, 3, 0, None, 0, None, None, None, 0, ctypes.byref(ns)) == -1
    assert L.pf_debug_fg_schedule(0, 3, 3, 1, None, 0, ctypes.byref(nr), None, None, 0, ctypes.byref(ns)) == 0      # N = 0 has a table too
