"""Host side of the down form of the 3x3 packed-pair kernel (plan option fold_down; no GPU): which ops of a table plan creation matches
and what it packs for them.  The fragments live in a region of their own (pf_debug_plan_down) beside the weight arena and the tail
region, which stay what tests/test_share_s_host.py and tests/test_fold_final_host.py pin them to whatever fold_down says."""
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
from test_fold_final_host import hard_block, k_channel, plan_tail, random_params
from test_share_s_host import option, plan_arena  # noqa: F401  (the fixture and the arena reader of the share / add tests)

TILES = 4                       # cout tiles of the reader the form packs, whatever the reader has
FRAG = TILES * 2 * 2 * 64 * 4   # floats: [tile][chunk][term][lane][8 fp16]


def plan_down(blob, in_ch, n_cls, n_ops):
    """(down region as float32 array, per op its offset in floats or 0) of the plan the library would create from the blob now"""
    L = pflib.load()
    buf = ctypes.create_string_buffer(blob, len(blob))
    n = ctypes.c_size_t()
    pflib.check(L.pf_debug_plan_down(buf, len(blob), in_ch, n_cls, None, 0, ctypes.byref(n), None, 0), 'pf_debug_plan_down')
    region = np.zeros(max(n.value, 1), dtype=np.float32)
    table = np.zeros(n_ops, dtype=np.int64)
    pflib.check(L.pf_debug_plan_down(buf, len(blob), in_ch, n_cls, region.ctypes.data, region.size, ctypes.byref(n), table.ctypes.data, n_ops),
                'pf_debug_plan_down')
    return region[:n.value], table


def down_net(g, c_odd, c_even, r_cout, lead=0, c0=24, r_relu=True, pool=True, skip=False, cin0=12):
    """test_fold_final_host.hard_block over the input; behind it `dn` = a 1x1 conv with ReLU over the block's output, `pl` = its 2x2 average
    pool, `nx` = a 3x3 conv over the pooled tensor and, with `skip`, `sk` = a second reader of the block's output"""
    from helpers import MiniSpec
    S = arch.Src
    spec, shapes = MiniSpec(cin0), []
    out, out_ch = hard_block(spec, shapes, S(0, 0, cin0), c_odd, c_even, lead, c0)
    dn = spec.conv('dn', [S(out, 0, out_ch)], r_cout, 1, relu=r_relu)
    pl = spec.pool('pl', dn) if pool else dn
    spec.conv('nx', [S(pl, 0, r_cout)], 8, 3)
    shapes += [('dn', out_ch, r_cout, 1), ('nx', r_cout, 8, 3)]
    if skip:
        spec.conv('sk', [S(out, 0, out_ch)], 6, 1, relu=False)
        shapes += [('sk', out_ch, 6, 1)]
    return spec, random_params(g, shapes)


def both_net(g):
    """both fold forms in one table: FC-HarDNet-70's first block (10, 28) with its transition `dn` (64 couts) + `pl`, and behind the pool,
    in place of `nx`, its last block (10, 28) - names prefixed 'u.' - with `fin` (11 couts, no ReLU) over that block's output"""
    from helpers import MiniSpec
    S = arch.Src
    spec, shapes = MiniSpec(12), []
    out, out_ch = hard_block(spec, shapes, S(0, 0, 12), 10, 28)
    pl = spec.pool('pl', spec.conv('dn', [S(out, 0, out_ch)], 64, 1))
    shapes += [('dn', out_ch, 64, 1)]
    up, up_ch = hard_block(spec, shapes, S(pl, 0, 64), 10, 28, pre='u.')
    spec.conv('fin', [S(up, 0, up_ch)], 11, 1, relu=False)
    shapes += [('fin', up_ch, 11, 1)]
    return spec, random_params(g, shapes)


def own_packing(blob, spec, name, cout):
    """the 1x1 conv's own packed-pair weights: [cout tile][round][term][lane][8] fp16"""
    names = [op.name for op in spec.ops]
    arena, atab = plan_arena(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    s4_off, rounds = int(atab[names.index(name)][0]), int(atab[names.index(name)][1])
    tiles = (cout + 15) // 16
    return arena[s4_off:s4_off + tiles * rounds * 2 * 64 * 4].view(np.float16).reshape(tiles, rounds, 2, 64, 8)


def assert_equals_own_packing(got, own, front, c_even, r_cout):
    """got [tile][chunk][term][lane][8] against the reader's own packing term for term: entry j of its K order = group j of `out`;
    returns the number of (cout, channel) pairs compared"""
    n = 0
    for t in range(TILES):
        for chunk in range(2):
            for lane in range(64):
                for e in range(8):
                    ci = k_channel(chunk, lane >> 4, e, front, c_even)
                    if ci is None or 16 * t + (lane & 15) >= r_cout:
                        continue
                    ent = ci // 4
                    for term in range(2):
                        assert got[t, chunk, term, lane, e] == own[t, ent // 8, term, (lane & 15) + 16 * ((ent % 8) // 2), 4 * (ent % 2) + (ci & 3)]
                    n += 1
    return n


@pytest.mark.parametrize('c_odd,c_even,r_cout', [(10, 28, 64), (10, 18, 40), (12, 32, 16), (16, 20, 33)])
def test_fragments_hold_the_readers_weights_at_the_k_positions_the_kernel_reads(c_odd, c_even, r_cout, option):
    """hi + mid of every (cout, channel) of `dn` is its weight times 2^k to 2^-21 of max |w| at the K position of that channel, every other
    value of the four tiles' two chunks is zero (rows past dn's couts, K positions past the ranges), the fragments sit on the 3x3 op and
    equal dn's own packing term for term"""
    option('normalize_ranges', 0, 1)
    option('fold_down', 2, 1)
    g = torch.Generator().manual_seed(c_even + r_cout)
    spec, P = down_net(g, c_odd, c_even, r_cout)
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    region, table = plan_down(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    names = [op.name for op in spec.ops]
    assert [names[i] for i in np.nonzero(table)[0]] == ['L4']
    off = int(table[names.index('L4')])
    assert off >= 64 and off % 16 == 0 and not region[:64].any() and region.size == off + FRAG
    got = region[off:off + FRAG].view(np.float16).reshape(TILES, 2, 2, 64, 8)   # [tile][chunk][term][lane][e]
    h = got.astype(np.float64)
    val = h[:, :, 0] + h[:, :, 1]
    front, cin = 2 * c_odd, 2 * c_odd + c_even
    wt = P['dn'][0].double().numpy().reshape(r_cout, cin)
    k = 14 - int(np.floor(np.log2(np.abs(wt).max())))
    seen = np.zeros((r_cout, cin), dtype=np.int32)
    for t in range(TILES):
        for chunk in range(2):
            for lane in range(64):
                co, grp = 16 * t + (lane & 15), lane >> 4
                for e in range(8):
                    ci = k_channel(chunk, grp, e, front, c_even)
                    if co < r_cout and ci is not None:
                        assert abs(val[t, chunk, lane, e] * 2.0 ** -k - wt[co, ci]) <= 2.0 ** -21 * np.abs(wt).max(), (t, chunk, lane, e)
                        seen[co, ci] += 1
                    else:
                        assert h[t, chunk, 0, lane, e] == 0.0 and h[t, chunk, 1, lane, e] == 0.0, (t, chunk, lane, e)
    assert (seen == 1).all()      # every weight once, none in two slots
    assert assert_equals_own_packing(got, own_packing(blob, spec, 'dn', r_cout), front, c_even, r_cout) == r_cout * cin


def test_channel_scales_are_folded_in(option):
    """with the plan's power-of-two channel scales on, the fragments equal dn's own packing entry for entry all the same"""
    option('fold_down', 2, 1)
    g = torch.Generator().manual_seed(3)
    spec, P = down_net(g, 10, 28, 64)
    P['L1'] = (P['L1'][0] * 64.0, P['L1'][1] * 64.0)      # a slice the plan stores scaled down
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    region, table = plan_down(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    names = [op.name for op in spec.ops]
    off = int(table[names.index('L4')])
    got = region[off:off + FRAG].view(np.float16).reshape(TILES, 2, 2, 64, 8)
    assert assert_equals_own_packing(got, own_packing(blob, spec, 'dn', 64), 20, 28, 64) == 64 * 48
    # ... and differ from the packing without the scales: the check above is not vacuous
    option('normalize_ranges', 0, 1)
    raw, rtab = plan_down(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    assert not np.array_equal(raw[int(rtab[names.index('L4')]):].view(np.uint16), region[off:].view(np.uint16))


@pytest.mark.parametrize('kw', [dict(lead=2), dict(r_relu=False), dict(r_cout=65), dict(pool=False), dict(c_even=16), dict(c_even=36),
                                dict(c_odd=18)],
                         ids=['slice_in_mid_group', 'no_relu', '65_couts', 'no_pool', 'one_cout_tile', 'three_cout_tiles', '36_in_front'])
def test_tables_the_pattern_refuses(kw, option):
    option('fold_down', 2, 1)
    args = dict(c_odd=10, c_even=28, r_cout=64)
    args.update(kw)
    spec, P = down_net(torch.Generator().manual_seed(1), **args)
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    region, table = plan_down(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    assert region.size == 0 and not table.any()


def test_other_readers_of_the_slice_are_allowed(option):
    option('fold_down', 2, 1)
    spec, P = down_net(torch.Generator().manual_seed(1), 10, 28, 64, skip=True)
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    region, table = plan_down(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    assert region.size == 64 + FRAG and [spec.ops[i].name for i in np.nonzero(table)[0]] == ['L4']


def test_plan_created_with_fold_down_off_packs_nothing(option):
    """... and neither the arena nor the tail region knows the option"""
    spec, P = down_net(torch.Generator().manual_seed(1), 10, 28, 64)
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    tspec, tP = __import__('test_fold_final_host').tail_net(torch.Generator().manual_seed(1), 10, 28, 11)
    tblob = packing.pack_blob(None, tspec.in_ch, tspec.n_cls, spec=tspec, params=tP)
    seen = {}
    for mode in (0, 1, 2):
        option('fold_down', mode, 1)
        region, table = plan_down(blob, spec.in_ch, spec.n_cls, len(spec.ops))
        if mode == 0:
            assert region.size == 0 and not table.any()
        else:
            assert region.size == 64 + FRAG and np.count_nonzero(table) == 1
        seen[mode] = (plan_arena(blob, spec.in_ch, spec.n_cls, 1)[0], plan_arena(tblob, tspec.in_ch, tspec.n_cls, 1)[0],
                      plan_tail(tblob, tspec.in_ch, tspec.n_cls, len(tspec.ops))[0])
        assert seen[mode][2].size == 64 + 2 * 2 * 64 * 4
    for mode in (1, 2):
        for a, b in zip(seen[0], seen[mode]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_fchardnet70_matches_the_first_block_and_its_transition_only(option):
    option('fold_down', 2, 1)
    with open(os.path.join(GOLDEN, 'calib_seed1234.json')) as f:
        sd = synth.make_state_dict(seed=1234, calib=json.load(f))
    blob = packing.pack_blob(sd, 36, 11)
    spec = arch.Spec(36, 11)
    region, table = plan_down(blob, 36, 11, len(spec.ops))
    hits = np.nonzero(table)[0].tolist()
    assert len(hits) == 1
    i = hits[0]
    assert spec.ops[i].name == 'base.4.layers.3' and spec.ops[i + 1].name == 'base.5' and spec.ops[i + 2].kind == arch.OP_POOL
    assert (spec.ops[i].cin, spec.ops[i].cout, spec.ops[i + 1].cin, spec.ops[i + 1].cout) == (76, 28, 48, 64)
    assert region.size == 64 + FRAG


def test_both_forms_in_one_table(option):
    """a down block whose pooled transition feeds a tail block: each form's region holds one packing, on that block's last 3x3 layer"""
    option('fold_final', 2, 1)
    option('fold_down', 2, 1)
    spec, P = both_net(torch.Generator().manual_seed(1))
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    names = [op.name for op in spec.ops]
    tail, ttab = plan_tail(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    down, dtab = plan_down(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    assert [names[i] for i in np.nonzero(ttab)[0]] == ['u.L4'] and names[names.index('u.L4') + 1] == 'fin'
    assert [names[i] for i in np.nonzero(dtab)[0]] == ['L4'] and names[names.index('L4') + 1:names.index('L4') + 3] == ['dn', 'pl']
    assert tail.size == 64 + 2 * 2 * 64 * 4 and down.size == 64 + FRAG
