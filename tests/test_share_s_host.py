"""Host side of the share / add launches (plan option share_s; no GPU): what plan creation packs for them."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from panoptic_forecasting_amd import lib as pflib
from panoptic_forecasting_amd import packing, synth

TAP3 = ((0, 1, 3, 4), (6, 7, 2, 5))   # ky * 3 + kx of (instruction, lane group): csrc/conv_pack.cpp, pack_conv_weights_s4


@pytest.fixture
def option():
    """process-wide options for the plans a test creates; the library's defaults afterwards"""
    L = pflib.load()
    touched = {}

    def set_(name, value, default):
        touched[name] = default
        pflib.check(L.pf_set_option(name.encode(), value), 'pf_set_option')
    yield set_
    for name, default in touched.items():
        pflib.check(L.pf_set_option(name.encode(), default), 'pf_set_option')


def plan_arena(blob, in_ch, n_cls, n_ops):
    """(arena as float32 array, table [n_ops][6]) of the plan the library would create from the blob now"""
    L = pflib.load()
    buf = ctypes.create_string_buffer(blob, len(blob))
    n = ctypes.c_size_t()
    pflib.check(L.pf_debug_plan_arena(buf, len(blob), in_ch, n_cls, None, 0, ctypes.byref(n), None, 0), 'pf_debug_plan_arena')
    arena = np.zeros(n.value, dtype=np.float32)
    table = np.zeros((n_ops, 6), dtype=np.int64)
    pflib.check(L.pf_debug_plan_arena(buf, len(blob), in_ch, n_cls, arena.ctypes.data, arena.size, ctypes.byref(n), table.ctypes.data, n_ops),
                'pf_debug_plan_arena')
    return arena, table


def unpack_s4_3x3(arena, off, cout, cin, ranges, cstart):
    """inverse of pack_conv_weights_s4 for a 3x3 conv without padded ranges: [cout][cin][9] float64 of hi + mid.  ranges = (choff, ch)
    of every source range in the packed order, cstart = its first channel in the conv's input numbering"""
    ent = []                      # (conv channel of the group's channel 0, lo, hi)
    for (choff, ch), c0 in zip(ranges, cstart):
        for g in range(choff // 4, (choff + ch + 3) // 4):
            ent.append((c0 + 4 * g - choff, c0, c0 + ch))
    rounds, ntiles = (len(ent) + 1) // 2, (cout + 15) // 16
    h = arena[off:].view(np.float16)
    w = np.zeros((cout, cin, 9))
    seen = np.zeros((cout, cin, 9), dtype=np.int32)
    o = 0
    for t in range(ntiles):
        for rd in range(rounds):
            blocks = [(lambda g, hh, rd=rd: rd * 2 + hh, lambda g, s=s: TAP3[s][g]) for s in range(2)]
            if rd % 4 == 3 or rd == rounds - 1:
                q = rd // 4
                blocks.append((lambda g, hh, q=q: (4 * q + g) * 2 + hh if 4 * q + g < rounds else -1, lambda g: 8))
            for ent_of, tap_of in blocks:
                blk = h[o:o + 2 * 64 * 8].astype(np.float64).reshape(2, 64, 8)
                o += 2 * 64 * 8
                val = blk[0] + blk[1]
                for lane in range(64):
                    co, g = t * 16 + (lane & 15), lane >> 4
                    for e in range(8):
                        en, ok = ent_of(g, e // 4), False
                        if co < cout and 0 <= en < len(ent):
                            ci = ent[en][0] + (e & 3)
                            ok = ent[en][1] <= ci < ent[en][2]
                        if ok:
                            w[co, ci, tap_of(g)] += val[lane, e]
                            seen[co, ci, tap_of(g)] += 1
                        else:
                            assert val[lane, e] == 0.0
    assert (seen <= 1).all()      # no weight sits in two slots of the stream
    return w, seen


@pytest.mark.parametrize('c_odd,c_even,deep', [(10, 18, False), (12, 20, True), (6, 10, False), (18, 30, True)])
def test_share_and_add_packings_hold_the_consumers_weights_once(c_odd, c_even, deep, option):
    """The share launch's rows from roundup4(P couts) on, over the columns of S, and the add launch's packing over the other columns
    are, added, exactly the consumer's own packed weights (same fp16 terms, same power-of-two scale), and the share launch's first
    rows exactly the odd layer's; without range normalisation those are the network's weights times 2^k to 2^-21."""
    from test_gpu_share_s import pair_net
    option('normalize_ranges', 0, 1)
    g = torch.Generator().manual_seed(c_even)
    spec, P = pair_net(g, 12, c_odd, c_even, deep)
    blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=P)
    arena, table = plan_arena(blob, spec.in_ch, spec.n_cls, len(spec.ops))
    names = [op.name for op in spec.ops]
    n_pairs = 0
    for i, op in enumerate(spec.ops):
        s4_off, s4_rounds, a_off, a_tiles, b_off, b_rounds = table[i]
        if not a_off:
            continue
        n_pairs += 1
        p = spec.ops[i - 1]
        assert names[i] in ('L2', 'L4', 'L6', 'L8') and b_off and op.srcs[1].tensor == p.srcs[0].tensor
        rng = [(s.choff, s.ch) for s in op.srcs]
        c0 = np.cumsum([0] + [s.ch for s in op.srcs]).tolist()
        whole, seen = unpack_s4_3x3(arena, s4_off, op.cout, op.cin, rng, c0[:-1])
        assert seen.all()
        row0 = (p.cout + 3) // 4 * 4
        assert a_tiles == (row0 + op.cout + 15) // 16
        a, seen_a = unpack_s4_3x3(arena, a_off, row0 + op.cout, p.cin, [(p.srcs[0].choff, p.srcs[0].ch)], [0])
        b, seen_b = unpack_s4_3x3(arena, b_off, op.cout, op.cin, [rng[0]] + rng[2:], [c0[0]] + c0[2:-1])
        assert seen_a.all() and not seen_b[:, c0[1]:c0[2]].any() and seen_b[:, :c0[1]].all() and seen_b[:, c0[2]:].all()
        assert a[row0:].any() and b.any()
        summed = b.copy()
        summed[:, c0[1]:c0[2]] += a[row0:]
        assert np.array_equal(summed, whole), names[i]
        assert not a[p.cout:row0].any()
        p_whole, _ = unpack_s4_3x3(arena, table[i - 1][0], p.cout, p.cin, [(p.srcs[0].choff, p.srcs[0].ch)], [0])
        assert np.array_equal(a[:p.cout], p_whole), names[i - 1]
        wt = P[names[i]][0].double().numpy().reshape(op.cout, op.cin, 9)
        k = 14 - int(np.floor(np.log2(np.abs(wt).max())))
        assert np.abs(whole * 2.0 ** -k - wt).max() <= 2.0 ** -21 * np.abs(wt).max()
    assert n_pairs == (4 if deep else 2)


def test_plans_created_with_share_s_off_pack_what_they_packed_before(option):
    """FC-HarDNet-70: the weight arena of a plan created under share_s = 0 is byte for byte the arena of the library before the share /
    add launches existed (tests/golden/arena_fchardnet70_seed1234.json: its size and SHA-256); with share_s = 1 it only grows, to the arena
    recorded under the library's default options at 56bf59a (default_floats, default_sha256: the share and add packings included), before
    the packers took the order of their ranges from csrc/conv_ranges.cpp."""
    with open(os.path.join(GOLDEN, 'calib_seed1234.json')) as f:
        sd = synth.make_state_dict(seed=1234, calib=json.load(f))
    blob = packing.pack_blob(sd, 36, 11)
    with open(os.path.join(GOLDEN, 'arena_fchardnet70_seed1234.json')) as f:
        want = json.load(f)
    option('share_s', 0, 1)
    off, _ = plan_arena(blob, 36, 11, 1)
    assert off.size == want['floats']
    assert hashlib.sha256(off.tobytes()).hexdigest() == want['sha256']
    option('share_s', 1, 1)
    on, _ = plan_arena(blob, 36, 11, 1)
    assert on.size > off.size
    assert on.size == want['default_floats']
    assert hashlib.sha256(on.tobytes()).hexdigest() == want['default_sha256']
