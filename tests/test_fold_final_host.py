"""Host side of the tail form of the 3x3 packed-pair kernel (plan option fold_final; no GPU): which ops of a table plan creation matches
and what it packs for them.  The fragments live in a region of their own beside the weight arena (pf_debug_plan_tail): the arena of a plan
stays what tests/test_share_s_host.py pins it to whatever fold_final says."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from panoptic_forecasting_amd import hardnet_arch as arch
from panoptic_forecasting_amd import lib as pflib
from panoptic_forecasting_amd import packing, synth
from test_share_s_host import option, plan_arena  # noqa: F401  (the fixture and the arena reader of the share / add tests)


def plan_tail(blob, in_ch, n_cls, n_ops):
    """(tail region as float32 array, per op its offset in floats or 0) of the plan the library would create from the blob now"""
    L = pflib.load()
    buf = ctypes.create_string_buffer(blob, len(blob))
    n = ctypes.c_size_t()
    pflib.check(L.pf_debug_plan_tail(buf, len(blob), in_ch, n_cls, None, 0, ctypes.byref(n), None, 0), 'pf_debug_plan_tail')
    region = np.zeros(max(n.value, 1), dtype=np.float32)
    table = np.zeros(n_ops, dtype=np.int64)
    pflib.check(L.pf_debug_plan_tail(buf, len(blob), in_ch, n_cls, region.ctypes.data, region.size, ctypes.byref(n), table.ctypes.data, n_ops),
                'pf_debug_plan_tail')
    return region[:n.value], table


def k_channel(chunk, g, e, front, cout):
    """channel of the reader's range at K position e of lane group g - what the kernel multiplies there (csrc/conv_s4_kernel.inc, tail):
    chunk 0 = channel e & 3 of group entry 2g + e // 4 of the channels in front of the slice, chunk 1 = cout 4g + (e & 3) of the producing
    launch's cout tile e // 4, behind them; None = nothing"""
    if chunk == 0:
        c = 4 * (2 * g + e // 4) + (e & 3)
        return c if c < front else None
    c = 16 * (e // 4) + 4 * g + (e & 3)
    return front + c if c < cout else None


def hard_block(spec, shapes, src, c_odd, c_even, lead=0, c0=24, pre=''):
    """`t0` = a 3x3 conv of the range `src`, then the block of test_gpu_share_s.pair_net over it with slots [L0,] L1, L3, L4 in the tensor
    `out` (names prefixed with `pre`); appends (name, cin, cout, k) of its convs to `shapes`; returns (out, its channels)"""
    S = arch.Src
    t0 = spec.conv(pre + 't0', [src], c0, 3)
    out_ch = lead + 2 * c_odd + c_even
    out = spec.tensor(pre + 'out', out_ch)
    shapes += [(pre + 't0', src.ch, c0, 3)]
    if lead:
        spec.conv(pre + 'L0', [S(t0, 0, c0)], lead, 3, dst=out, dst_choff=0)
        shapes += [(pre + 'L0', c0, lead, 3)]
    spec.conv(pre + 'L1', [S(t0, 0, c0)], c_odd, 3, dst=out, dst_choff=lead)
    l2 = spec.conv(pre + 'L2', [S(out, lead, c_odd), S(t0, 0, c0)], c_even, 3)
    spec.conv(pre + 'L3', [S(l2, 0, c_even)], c_odd, 3, dst=out, dst_choff=lead + c_odd)
    spec.conv(pre + 'L4', [S(out, lead + c_odd, c_odd), S(l2, 0, c_even), S(t0, 0, c0)], c_even, 3, dst=out, dst_choff=lead + 2 * c_odd)
    shapes += [(pre + 'L1', c0, c_odd, 3), (pre + 'L2', c_odd + c0, c_even, 3), (pre + 'L3', c_even, c_odd, 3),
               (pre + 'L4', c_odd + c_even + c0, c_even, 3)]
    return out, out_ch


def random_params(g, shapes):
    return {n: (torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5, torch.randn(co, generator=g) * 0.5) for n, ci, co, k in shapes}


def tail_net(g, c_odd, c_even, fin_cout, lead=0, c0=24, fin_relu=False, second_reader=False, cin0=12):
    """hard_block over the input and `fin` = a 1x1 conv over the block's output"""
    from helpers import MiniSpec
    S = arch.Src
    spec, shapes = MiniSpec(cin0), []
    out, out_ch = hard_block(spec, shapes, S(0, 0, cin0), c_odd, c_even, lead, c0)
    spec.conv('fin', [S(out, 0, out_ch)], fin_cout, 1, relu=fin_relu)
    shapes += [('fin', out_ch, fin_cout, 1)]
    if second_reader:
        spec.conv('side', [S(out, 0, out_ch)], 6, 1, relu=False)
        shapes += [('side', out_ch, 6, 1)]
    return spec, random_params(g, shapes)


@pytest.mark.parametrize('c_odd,c_even,fin_cout', [(10, 28, 11), (10, 18, 5), (12, 32, 16), (16, 20, 1)])
def test_fragments_hold_the_readers_weights_at_the_k_positions_the_kernel_reads(c_odd, c_even, fin_cout, option):
    """hi + mid of every (cout, channel) of `fin` is its weight times 2^k to 2^-21 at the K position of that channel, every other value
    of the two chunks is zero (rows past fin's couts, K positions past the ranges), and the fragments sit on the 3x3 op"""
    option('normalize_ranges', 0, 1)
    g = torch.Generator().manual_seed(c_even + fin_cout)
    spec, P = tail_net(g, c_odd, c_even, fin_cout)
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    region, table = plan_tail(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    names = [op.name for op in spec.ops]
    assert [names[i] for i in np.nonzero(table)[0]] == ['L4']
    off = int(table[names.index('L4')])
    assert off >= 64 and off % 16 == 0 and not region[:64].any()
    h = region[off:off + 2 * 2 * 64 * 4].view(np.float16).astype(np.float64).reshape(2, 2, 64, 8)   # [chunk][term][lane][e]
    val = h[:, 0] + h[:, 1]
    front, cin = 2 * c_odd, 2 * c_odd + c_even
    wt = P['fin'][0].double().numpy().reshape(fin_cout, cin)
    k = 14 - int(np.floor(np.log2(np.abs(wt).max())))
    seen = np.zeros((fin_cout, cin), dtype=np.int32)
    for chunk in range(2):
        for lane in range(64):
            co, grp = lane & 15, lane >> 4
            for e in range(8):
                ci = k_channel(chunk, grp, e, front, c_even)
                if co < fin_cout and ci is not None:
                    assert abs(val[chunk, lane, e] * 2.0 ** -k - wt[co, ci]) <= 2.0 ** -21 * np.abs(wt).max(), (chunk, lane, e)
                    seen[co, ci] += 1
                else:
                    assert h[chunk, 0, lane, e] == 0.0 and h[chunk, 1, lane, e] == 0.0, (chunk, lane, e)
    assert (seen == 1).all()      # every weight once, none in two slots
    # the same fp16 terms as fin's own 1x1 packing holds (same scale): entry j of its K order = group j of `out`
    arena, atab = plan_arena(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    s4_off, rounds = int(atab[names.index('fin')][0]), int(atab[names.index('fin')][1])
    own = arena[s4_off:s4_off + rounds * 2 * 64 * 4].view(np.float16).reshape(rounds, 2, 64, 8)   # one cout tile: [round][term][lane][8]
    for chunk in range(2):
        for lane in range(64):
            for e in range(8):
                ci = k_channel(chunk, lane >> 4, e, front, c_even)
                if ci is None or (lane & 15) >= fin_cout:
                    continue
                ent = ci // 4
                src_lane = (lane & 15) + 16 * ((ent % 8) // 2)
                for term in range(2):
                    assert region[off:].view(np.float16).reshape(-1, 2, 64, 8)[chunk, term, lane, e] == own[ent // 8, term, src_lane, 4 * (ent % 2) + (ci & 3)]


def test_channel_scales_are_folded_in(option):
    """with the plan's power-of-two channel scales on, the fragments equal fin's own packing entry for entry all the same (the check above,
    without the comparison against the raw weights)"""
    g = torch.Generator().manual_seed(3)
    spec, P = tail_net(g, 10, 28, 11)
    P['L1'] = (P['L1'][0] * 64.0, P['L1'][1] * 64.0)      # a slice the plan stores scaled down
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    region, table = plan_tail(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    names = [op.name for op in spec.ops]
    off = int(table[names.index('L4')])
    arena, atab = plan_arena(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    s4_off, rounds = int(atab[names.index('fin')][0]), int(atab[names.index('fin')][1])
    own = arena[s4_off:s4_off + rounds * 2 * 64 * 4].view(np.float16).reshape(rounds, 2, 64, 8)
    got = region[off:off + 2 * 2 * 64 * 4].view(np.float16).reshape(2, 2, 64, 8)
    n = 0
    for chunk in range(2):
        for lane in range(64):
            for e in range(8):
                ci = k_channel(chunk, lane >> 4, e, 20, 28)
                if ci is None or (lane & 15) >= 11:
                    continue
                ent = ci // 4
                for term in range(2):
                    assert got[chunk, term, lane, e] == own[ent // 8, term, (lane & 15) + 16 * ((ent % 8) // 2), 4 * (ent % 2) + (ci & 3)]
                n += 1
    assert n == 11 * 48


@pytest.mark.parametrize('kw', [dict(lead=2), dict(fin_relu=True), dict(fin_cout=17), dict(second_reader=True), dict(c_even=16), dict(c_even=36),
                                dict(c_odd=18)])
def test_tables_the_pattern_refuses(kw, option):
    """a slice that starts in the middle of a group, a reader with ReLU, with 17 couts, a second reader, one and three cout tiles, more than
    32 channels in front of the slice: nothing is packed"""
    args = dict(c_odd=10, c_even=28, fin_cout=11)
    args.update(kw)
    spec, P = tail_net(torch.Generator().manual_seed(1), **args)
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    region, table = plan_tail(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    assert region.size == 0 and not table.any()


def test_plan_created_with_fold_final_off_packs_nothing(option):
    spec, P = tail_net(torch.Generator().manual_seed(1), 10, 28, 11)
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    on, _ = plan_arena(blob, spec.in_ch, spec.n_cls, 1)
    option('fold_final', 0, 1)
    region, table = plan_tail(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    assert region.size == 0 and not table.any()
    off, _ = plan_arena(blob, spec.in_ch, spec.n_cls, 1)
    assert np.array_equal(on, off)          # the arena does not know the option
    option('fold_final', 2, 1)
    region, table = plan_tail(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    assert region.size == 64 + 2 * 2 * 64 * 4 and np.count_nonzero(table) == 1


def test_fchardnet70_matches_the_last_decoder_layer_and_finalconv_only():
    with open(os.path.join(GOLDEN, 'calib_seed1234.json')) as f:
        sd = synth.make_state_dict(seed=1234, calib=json.load(f))
    blob = packing.pack_blob(sd, 36, 11)
    spec = arch.Spec(36, 11)
    region, table = plan_tail(blob, 36, 11, len(spec.ops))
    hits = np.nonzero(table)[0].tolist()
    assert len(hits) == 1
    i = hits[0]
    assert spec.ops[i].name == 'denseBlocksUp.3.layers.3' and spec.ops[i + 1].name == 'finalConv'
    assert (spec.ops[i].cin, spec.ops[i].cout, spec.ops[i + 1].cin, spec.ops[i + 1].cout) == (91, 28, 48, 11)
    assert region.size == 64 + 2 * 2 * 64 * 4
