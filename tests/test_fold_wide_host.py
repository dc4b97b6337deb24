"""Host side of the fold forms of three-tile producers (no GPU): down3 - plan option fold_down, a 3x3 conv of 33 .. 48 couts in front of
a 1x1 conv with ReLU of at most 96 couts and its 2x2 average pool - and lo - plan option fold_lo, the same producer in front of an
upsample + 1x1 conv pair whose low-resolution half the schedule runs on its own.  Which ops of a table plan creation matches, what it
packs for them - into regions of their own (pf_debug_plan_wide), cout tile by cout tile, three K = 32 chunks per tile - and that the
weight arena, the tail region and the down region stay byte for byte what they are.  (Which launches the schedule folds - K-split
shapes, the add launch of a share pair, the rule - is read from the step list, without a device: tests/test_hardnet_schedule_host.py;
the numbers of the folded launches: tests/test_gpu_fold_wide.py.)"""
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
from test_fold_down_host import down_net, own_packing, plan_down
from test_fold_final_host import hard_block, plan_tail, random_params
from test_share_s_host import option, plan_arena  # noqa: F401  (the fixture and the arena reader of the share / add tests)

DOWN3, LO = 2, 3                          # FoldForm (csrc/conv_mfma.h)
TILES = {DOWN3: 6, LO: 4}                 # cout tiles of the reader the form packs, whatever the reader has
OPTION = {DOWN3: 'fold_down', LO: 'fold_lo'}


def frag_floats(form):
    return TILES[form] * 3 * 2 * 64 * 4   # [tile][chunk 3][term][lane][8 fp16]


def plan_wide(form, blob, in_ch, n_cls, n_ops):
    """(the form's region as float32 array, per op its offset in floats or 0) of the plan the library would create from the blob now"""
    L = pflib.load()
    buf = ctypes.create_string_buffer(blob, len(blob))
    n = ctypes.c_size_t()
    pflib.check(L.pf_debug_plan_wide(form, buf, len(blob), in_ch, n_cls, None, 0, ctypes.byref(n), None, 0), 'pf_debug_plan_wide')
    region = np.zeros(max(n.value, 1), dtype=np.float32)
    table = np.zeros(n_ops, dtype=np.int64)
    pflib.check(L.pf_debug_plan_wide(form, buf, len(blob), in_ch, n_cls, region.ctypes.data, region.size, ctypes.byref(n), table.ctypes.data,
                                     n_ops), 'pf_debug_plan_wide')
    return region[:n.value], table


def k_channel3(chunk, g, e, front, cout):
    """channel of the reader's range at K position e of lane group g, three-tile producers: chunk 0 = channel e & 3 of group entry
    2g + e // 4 of the channels in front of the slice; chunk 1 = cout 4g + (e & 3) of the producing launch's cout tile e // 4; chunk 2 =
    cout 4g + e of its cout tile 2 at e < 4, nothing above (a lane's D fragments are 4 couts of one pixel per cout tile); None = nothing"""
    if chunk == 0:
        c = 4 * (2 * g + e // 4) + (e & 3)
        return c if c < front else None
    if chunk == 2 and e >= 4:
        return None
    c = 16 * (e // 4) + 4 * g + (e & 3) if chunk == 1 else 32 + 4 * g + e
    return front + c if c < cout else None


def lo_net(g, c_odd, c_even, r_cout, lead=0, skip_ch=12, second_reader=False, side=False, cin0=12):
    """`hi` = a 3x3 conv over the input (the skip tensor), `s2` = a 3x3 stride-2 conv over the input, test_fold_final_host.hard_block over
    `s2`; behind it `up` = the upsample of the block's output to hi's size, `cu` = a 1x1 conv with ReLU over [up, hi] and `nx` = a 3x3
    conv over cu.  `second_reader`: `sk`, a 1x1 conv at the low resolution, reads the block's output too; `side`: `sd` reads `up`"""
    from helpers import MiniSpec
    S = arch.Src
    spec, shapes = MiniSpec(cin0), []
    hi = spec.conv('hi', [S(0, 0, cin0)], skip_ch, 3)
    s2 = spec.conv('s2', [S(0, 0, cin0)], 16, 3, stride=2)
    shapes += [('hi', cin0, skip_ch, 3), ('s2', cin0, 16, 3)]
    out, out_ch = hard_block(spec, shapes, S(s2, 0, 16), c_odd, c_even, lead)
    up = spec.upsample('up', out, hi)
    cu = spec.conv('cu', [S(up, 0, out_ch), S(hi, 0, skip_ch)], r_cout, 1)
    spec.conv('nx', [S(cu, 0, r_cout)], 8, 3)
    shapes += [('cu', out_ch + skip_ch, r_cout, 1), ('nx', r_cout, 8, 3)]
    if second_reader:
        spec.conv('sk', [S(out, 0, out_ch)], 6, 1, relu=False)
        shapes += [('sk', out_ch, 6, 1)]
    if side:
        spec.conv('sd', [S(up, 0, out_ch)], 6, 1, relu=False)
        shapes += [('sd', out_ch, 6, 1)]
    return spec, random_params(g, shapes)


def wide_net(form, g, c_odd, c_even, r_cout, **kw):
    """(spec, params, name of the reader) of the form's test network"""
    if form == DOWN3:
        return down_net(g, c_odd, c_even, r_cout, **kw) + ('dn',)
    return lo_net(g, c_odd, c_even, r_cout, **kw) + ('cu',)


# L couts 40 (eight channels in front of the slice: chunks 0 and 2 mostly zeros), 46 and 48 (32 in front: every K position of chunk 0 in
# use; 48: of chunk 2's low half too); reader couts 17 (its second tile holds one row), 63 and 96 (down3 only: six full tiles)
CASES = [(form, c_odd, c_even, r_cout) for form in (DOWN3, LO) for c_odd, c_even in ((4, 40), (16, 46), (16, 48)) for r_cout in (17, 63, 96)
         if not (form == LO and r_cout == 96)]


@pytest.mark.parametrize('form,c_odd,c_even,r_cout', CASES)
def test_fragments_hold_the_readers_weights_at_the_k_positions_the_kernel_reads(form, c_odd, c_even, r_cout, option):
    """hi + mid of every (cout, channel of the range) of the reader is its weight times 2^k to 2^-21 of max |w| at the K position of that
    channel, every other value of the tiles' three chunks is zero (rows past the reader's couts, K positions past the ranges, the upper
    half of chunk 2), the fragments sit on the 3x3 op, tile after tile, and equal the reader's own packing term for term"""
    option('normalize_ranges', 0, 1)
    option(OPTION[form], 2, 1)
    g = torch.Generator().manual_seed(c_even + r_cout)
    spec, P, reader = wide_net(form, g, c_odd, c_even, r_cout)
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    region, table = plan_wide(form, blob, spec.in_ch, spec.n_cls, len(spec.ops))
    names = [op.name for op in spec.ops]
    assert [names[i] for i in np.nonzero(table)[0]] == ['L4']
    off, tiles, n = int(table[names.index('L4')]), TILES[form], frag_floats(form)
    assert off >= 64 and off % 16 == 0 and not region[:64].any() and region.size == off + n
    got = region[off:off + n].view(np.float16).reshape(tiles, 3, 2, 64, 8)   # [tile][chunk][term][lane][e]
    h = got.astype(np.float64)
    val = h[:, :, 0] + h[:, :, 1]
    front, cin = 2 * c_odd, 2 * c_odd + c_even
    full = P[reader][0].double().numpy().reshape(r_cout, -1)
    k = 14 - int(np.floor(np.log2(np.abs(full).max())))      # (the reader's 2^k: over all of its columns)
    wt = full[:, :cin]                                       # lo: the columns of `up`, the first range
    own = own_packing(blob, spec, reader, r_cout)
    seen = np.zeros((r_cout, cin), dtype=np.int32)
    for t in range(tiles):
        for chunk in range(3):
            for lane in range(64):
                co, grp = 16 * t + (lane & 15), lane >> 4
                for e in range(8):
                    ci = k_channel3(chunk, grp, e, front, c_even)
                    if co < r_cout and ci is not None:
                        assert abs(val[t, chunk, lane, e] * 2.0 ** -k - wt[co, ci]) <= 2.0 ** -21 * np.abs(full).max(), (t, chunk, lane, e)
                        seen[co, ci] += 1
                        ent = ci // 4                        # entry of the reader's own K order = group of `out` (of `up`)
                        for term in range(2):
                            assert got[t, chunk, term, lane, e] == own[t, ent // 8, term, (lane & 15) + 16 * ((ent % 8) // 2), 4 * (ent % 2) + (ci & 3)]
                    else:
                        assert h[t, chunk, 0, lane, e] == 0.0 and h[t, chunk, 1, lane, e] == 0.0, (t, chunk, lane, e)
    assert (seen == 1).all()      # every weight once, none in two slots


def test_channel_scales_are_folded_in(option):
    """with the plan's power-of-two channel scales on, the fragments differ from the ones without them (and the test above holds for either:
    they are cut from the same scaled weights as the reader's own packing)"""
    for form in (DOWN3, LO):
        option(OPTION[form], 2, 1)
    for form in (DOWN3, LO):
        spec, P, reader = wide_net(form, torch.Generator().manual_seed(3), 16, 46, 63)
        P['L1'] = (P['L1'][0] * 64.0, P['L1'][1] * 64.0)      # a slice the plan stores scaled down
        blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
        names = [op.name for op in spec.ops]
        option('normalize_ranges', 1, 1)
        region, table = plan_wide(form, blob, spec.in_ch, spec.n_cls, len(spec.ops))
        off = int(table[names.index('L4')])
        got = region[off:].view(np.float16).reshape(TILES[form], 3, 2, 64, 8)
        own = own_packing(blob, spec, reader, 63)
        for lane in range(64):                                # chunk 0, K positions of L1's channels: entry 2g + e // 4 of the range
            for e in range(8):
                ci = k_channel3(0, lane >> 4, e, 32, 46)
                ent = ci // 4
                assert np.array_equal(got[:4, 0, :, lane, e], own[:4, ent // 8, :, (lane & 15) + 16 * ((ent % 8) // 2), 4 * (ent % 2) + (ci & 3)])
        option('normalize_ranges', 0, 1)
        raw, rtab = plan_wide(form, blob, spec.in_ch, spec.n_cls, len(spec.ops))
        assert not np.array_equal(raw[int(rtab[names.index('L4')]):].view(np.uint16), region[off:].view(np.uint16))


@pytest.mark.parametrize('form,kw', [(DOWN3, dict(lead=2)), (DOWN3, dict(r_relu=False)), (DOWN3, dict(r_cout=97)), (DOWN3, dict(pool=False)),
                                     (DOWN3, dict(c_even=28)), (DOWN3, dict(c_even=52)), (DOWN3, dict(c_odd=18)),
                                     (LO, dict(lead=2)), (LO, dict(r_cout=65)), (LO, dict(c_even=28)), (LO, dict(c_even=52)), (LO, dict(c_odd=18)),
                                     (LO, dict(side=True))],
                         ids=['down3-slice_in_mid_group', 'down3-no_relu', 'down3-97_couts', 'down3-no_pool', 'down3-two_cout_tiles', 'down3-four_cout_tiles',
                              'down3-36_in_front', 'lo-slice_in_mid_group', 'lo-65_couts', 'lo-two_cout_tiles', 'lo-four_cout_tiles', 'lo-36_in_front',
                              'lo-second_reader_of_the_upsample'])
def test_tables_the_pattern_refuses(form, kw, option):
    option('fold_down', 2, 1)
    option('fold_lo', 2, 1)
    args = dict(c_odd=16, c_even=46, r_cout=63)
    args.update(kw)
    spec, P, _ = wide_net(form, torch.Generator().manual_seed(1), **args)
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    region, table = plan_wide(form, blob, spec.in_ch, spec.n_cls, len(spec.ops))
    assert region.size == 0 and not table.any()


def test_reader_with_two_ranges_is_refused(option):
    """`dn` over [the block's output, t0]: its range does not end with the slice alone - neither down form packs anything"""
    from helpers import MiniSpec
    option('fold_down', 2, 1)
    S = arch.Src
    spec, shapes = MiniSpec(12), []
    out, out_ch = hard_block(spec, shapes, S(0, 0, 12), 16, 46)
    t0 = [i for i, t in enumerate(spec.tensors) if t.name == 't0'][0]
    pl = spec.pool('pl', spec.conv('dn', [S(out, 0, out_ch), S(t0, 0, 24)], 63, 1))
    spec.conv('nx', [S(pl, 0, 63)], 8, 3)
    P = random_params(torch.Generator().manual_seed(1), shapes + [('dn', out_ch + 24, 63, 1), ('nx', 63, 8, 3)])
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    for region, table in (plan_wide(DOWN3, blob, spec.in_ch, spec.n_cls, len(spec.ops)), plan_down(blob, spec.in_ch, spec.n_cls, len(spec.ops))):
        assert region.size == 0 and not table.any()


@pytest.mark.parametrize('form,kw', [(DOWN3, dict(skip=True)), (LO, dict(second_reader=True))], ids=['down3', 'lo'])
def test_other_readers_of_the_slice_are_allowed(form, kw, option):
    """(the schedule then stores the slice: tests/test_hardnet_schedule_host.py, tests/test_gpu_fold_wide.py)"""
    option(OPTION[form], 2, 1)
    spec, P, _ = wide_net(form, torch.Generator().manual_seed(1), 16, 46, 63, **kw)
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    region, table = plan_wide(form, blob, spec.in_ch, spec.n_cls, len(spec.ops))
    assert region.size == 64 + frag_floats(form) and [spec.ops[i].name for i in np.nonzero(table)[0]] == ['L4']


def test_arena_and_the_other_regions_do_not_know_the_options(option):
    """plans created with fold_down / fold_lo at 0, 1 and 2 over a down3 table, a lo table, a two-tile down table and a tail table: the
    wide regions are empty at 0 and hold one packing otherwise; the weight arena of all four, the tail region and the two-tile down
    region are the same bytes whatever the options say"""
    g = lambda: torch.Generator().manual_seed(1)
    nets = [wide_net(DOWN3, g(), 16, 46, 96)[:2], wide_net(LO, g(), 16, 46, 63)[:2], down_net(g(), 10, 28, 64),
            __import__('test_fold_final_host').tail_net(g(), 10, 28, 11)]
    blobs = [(packing.pack_blob(None, s.in_ch, s.n_cls, spec=s, params=P), s) for s, P in nets]
    seen = {}
    for mode in (0, 1, 2):
        option('fold_lo', mode, 1)
        for form, (blob, s) in zip((DOWN3, LO), blobs):
            region, table = plan_wide(form, blob, s.in_ch, s.n_cls, len(s.ops))
            if mode == 0 and form == LO:
                assert region.size == 0 and not table.any()
            else:
                assert region.size == 64 + frag_floats(form) and np.count_nonzero(table) == 1
        seen[mode] = [plan_arena(blob, s.in_ch, s.n_cls, 1)[0] for blob, s in blobs]
        seen[mode].append(plan_down(blobs[2][0], blobs[2][1].in_ch, 1, len(blobs[2][1].ops))[0])
        seen[mode].append(plan_tail(blobs[3][0], blobs[3][1].in_ch, 1, len(blobs[3][1].ops))[0])
        assert seen[mode][4].size == 64 + 4 * 2 * 2 * 64 * 4 and seen[mode][5].size == 64 + 2 * 2 * 64 * 4
    option('fold_down', 0, 1)
    blob, s = blobs[0]
    region, table = plan_wide(DOWN3, blob, s.in_ch, s.n_cls, len(s.ops))
    assert region.size == 0 and not table.any()
    seen[3] = [plan_arena(b, sp.in_ch, sp.n_cls, 1)[0] for b, sp in blobs] + seen[0][4:]
    for mode in (1, 2, 3):
        for a, b in zip(seen[0], seen[mode]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_fchardnet70_matches_the_second_block_down_and_the_third_decoder_block_up(option):
    option('fold_down', 2, 1)
    option('fold_lo', 2, 1)
    with open(os.path.join(GOLDEN, 'calib_seed1234.json')) as f:
        sd = synth.make_state_dict(seed=1234, calib=json.load(f))
    blob = packing.pack_blob(sd, 36, 11)
    spec = arch.Spec(36, 11)
    region, table = plan_wide(DOWN3, blob, 36, 11, len(spec.ops))
    hits = np.nonzero(table)[0].tolist()
    assert len(hits) == 1 and region.size == 64 + frag_floats(DOWN3)
    i = hits[0]
    assert spec.ops[i].name == 'base.7.layers.3' and spec.ops[i + 1].name == 'base.8' and spec.ops[i + 2].kind == arch.OP_POOL
    assert (spec.ops[i].cin, spec.ops[i].cout, spec.ops[i + 1].cin, spec.ops[i + 1].cout) == (108, 46, 78, 96)
    region, table = plan_wide(LO, blob, 36, 11, len(spec.ops))
    hits = np.nonzero(table)[0].tolist()
    assert len(hits) == 1 and region.size == 64 + frag_floats(LO)
    i = hits[0]
    assert spec.ops[i].name == 'denseBlocksUp.2.layers.3' and spec.ops[i + 1].kind == arch.OP_UPSAMPLE and spec.ops[i + 2].name == 'conv1x1_up.3'
    assert (spec.ops[i].cin, spec.ops[i].cout, spec.ops[i + 1].srcs[0].ch, spec.ops[i + 2].cout) == (163, 46, 78, 63)
    # the two-tile down region still holds the first block's transition only
    dreg, dtab = plan_down(blob, 36, 11, len(spec.ops))
    assert [spec.ops[j].name for j in np.nonzero(dtab)[0]] == ['base.4.layers.3'] and dreg.size == 64 + 4 * 2 * 2 * 64 * 4
