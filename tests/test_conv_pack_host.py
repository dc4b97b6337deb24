"""The weight layouts of the convolution kernels (csrc/conv_pack.cpp, through pf_debug_pack_conv): host code only, no GPU.

Every layout is restated here in numpy from the index formula of its doc comment and compared bit for bit (numpy.float16 rounds to nearest
even and keeps subnormals, as split_host_f16 does: tests/test_host_logic.py).  The buffer a writer gets is what its size function answers
plus 64 sentinel floats, all pre-filled with a NaN pattern no writer can produce from finite weights: the sentinels must survive and no
float in front of them may - a writer and its size function agree."""
import ctypes

import numpy as np
import pytest

from panoptic_forecasting_amd import lib as pflib

GENERIC, TILED, REM, WAVE, SPLIT, SPLIT1, S4, FOLD, PAIR_TWO, PAIR_NINE = range(10)
TAP3 = ((0, 1, 3, 4), (6, 7, 2, 5))   # ky * 3 + kx of (instruction, lane group) of a 3x3 packed-pair round; tap 8 is collected apart
FILL = 0x7fc07fc0                     # a NaN as fp32 and as each of its fp16 halves
COUTS = (5, 17)                       # one partial cout tile; a second tile with one row
LANE, E8 = np.ogrid[:64, :8]
N, G = LANE & 15, LANE >> 4           # a lane's cout inside the tile and its lane group


def weights(cout, cin, ks):
    """seeded [cout][cin][ks * ks] fp32 with, at both ends (the rem layout reads the last couts only): an exact zero, a value whose mid
    term is an fp16 subnormal, a value whose hi term is exact"""
    w = np.random.default_rng(cout * 1000 + cin * 10 + ks).standard_normal((cout, cin, ks * ks)).astype(np.float32)
    special = np.array([0.0, 1.0 + 2.0 ** -16, 0.5], dtype=np.float32)
    w.reshape(-1)[:3] = special
    w.reshape(-1)[-3:] = special
    hi = special.astype(np.float16)
    mid = (special - hi.astype(np.float32)).astype(np.float16)
    assert mid[1] != 0 and abs(float(mid[1])) < 2.0 ** -14 and mid[2] == 0 and hi[2] == special[2]
    return w


def gather(w, co, ci, tap):
    """w[co][ci][tap] over broadcast index arrays; 0 where co is past the conv's couts or ci is no channel of it (-1: padding)"""
    co, ci, tap = np.broadcast_arrays(co, ci, tap)
    ok = (co < w.shape[0]) & (ci >= 0) & (ci < w.shape[1])
    return np.where(ok, w[np.where(ok, co, 0), np.where(ok, ci, 0), tap], np.float32(0))


def pair_blocks(v):
    """[..., lane 64, E] fp32 -> the bytes of [...][term 2: hi, mid][lane][E] fp16"""
    hi = v.astype(np.float16)
    mid = (v - hi.astype(np.float32)).astype(np.float16)
    return np.stack([hi, mid], axis=-3).tobytes()


def chunked_k(src_ch, kc):
    """[chunk][kc] conv input channels of the K order 'the ranges in order, each padded to whole chunks'; -1 = padding"""
    k, c0 = [], 0
    for ch in src_ch:
        k += list(range(c0, c0 + ch)) + [-1] * (-ch % kc)
        c0 += ch
    return np.array(k).reshape(-1, kc)


def entries(ranges, per=1):
    """[entry][4] conv input channels of the group entries of (choff, ch) ranges: one per 4-channel group of its tensor a range touches,
    -1 where the range does not own the channel; every range padded to a multiple of `per` entries"""
    ent, c0 = [], 0
    for choff, ch in ranges:
        mine = [[c0 + c - choff if choff <= c < choff + ch else -1 for c in range(4 * g, 4 * g + 4)] for g in range(choff // 4, (choff + ch + 3) // 4)]
        ent += mine + [[-1] * 4] * (-len(mine) % per)
        c0 += ch
    return np.array(ent)


def ref_generic(w, ks, stride):
    cout, cin, ks2 = w.shape
    kc = 32 if ks == 1 else (8 if stride == 2 else 16)
    ntiles = (cout + 15) // 16
    nt = min(ntiles, 4)
    cb, chunk, kg, tap, n, lane = np.ogrid[:(ntiles + nt - 1) // nt, :(cin + kc - 1) // kc, :kc // 4, :ks2, :nt, :64]
    return gather(w, (cb * nt + n) * 16 + (lane & 15), chunk * kc + kg * 4 + (lane >> 4), tap).tobytes()


def ref_tiled(w, src_ch, kc):
    k = chunked_k(src_ch, kc)
    t, chunk, kg, tap, lane = np.ogrid[:(w.shape[0] + 15) // 16, :len(k), :kc // 4, :w.shape[2], :64]
    return gather(w, t * 16 + (lane & 15), k[chunk, kg * 4 + (lane >> 4)], tap).tobytes()


def ref_rem(w, src_ch, kc, rem):
    k, co0 = chunked_k(src_ch, kc), w.shape[0] - rem
    if rem <= 2:      # [chunk][kgroup][tap][2 couts][4 input channels]
        chunk, kg, tap, r, c = np.ogrid[:len(k), :kc // 4, :w.shape[2], :2, :4]
    else:             # [chunk][kgroup][tap][rv / 4][4 input channels][4 couts], rv = rem rounded up to 4
        chunk, kg, tap, g, c, q = np.ogrid[:len(k), :kc // 4, :w.shape[2], :(rem + 3) // 4, :4, :4]
        r = g * 4 + q
    return gather(w, co0 + r, k[chunk, kg * 4 + c], tap).tobytes()     # rows from rem on are past the conv's couts: zero


def ref_wave(w, src_ch, ks):
    kc, ks2 = (32 if ks == 1 else 8), ks * ks
    k, nv = chunked_k(src_ch, kc), kc // 4 * ks * ks
    nq, nr = nv // 4, nv % 4

    def val(idx, t, chunk, lane):
        return gather(w, t * 16 + (lane & 15), k[chunk, idx // ks2 * 4 + (lane >> 4)], idx % ks2)
    t, chunk, q, lane, e = np.ogrid[:(w.shape[0] + 15) // 16, :len(k), :nq, :64, :4]
    quads = val(q * 4 + e, t, chunk, lane)
    t, chunk, lane, e = np.ogrid[:(w.shape[0] + 15) // 16, :len(k), :64, :nr]
    rest = val(nq * 4 + e, t, chunk, lane)
    return np.concatenate([quads.reshape(quads.shape[:2] + (-1,)), rest.reshape(rest.shape[:2] + (-1,))], axis=2).tobytes(), nr


def ref_split(w, src_ch):
    k = chunked_k(src_ch, 8)
    t, chunk, s, lane, e = np.ogrid[:(w.shape[0] + 15) // 16, :len(k), :3, :64, :8]
    tap = 4 * s + (lane >> 4)
    return pair_blocks(np.where(tap < 9, gather(w, t * 16 + (lane & 15), k[chunk, e], np.minimum(tap, 8)), np.float32(0)))


def ref_split1(w, src_ch):
    k = chunked_k(src_ch, 32)
    t, chunk, lane, e = np.ogrid[:(w.shape[0] + 15) // 16, :len(k), :64, :8]
    return pair_blocks(gather(w, t * 16 + (lane & 15), k[chunk, (lane >> 4) * 8 + e], 0))


def ref_s4(w, ks, ranges, pad):
    per = 2 if ks == 3 else 8
    ent = entries(ranges, per if pad else 1)
    rounds = (len(ent) + per - 1) // per
    ent = np.concatenate([ent, np.full((4 * per * rounds, 4), -1)])      # entries past the last one: no channel

    def block(t, ent_of_g_h, tap_of_g):
        return pair_blocks(gather(w, t * 16 + N, ent[ent_of_g_h(G, E8 // 4), E8 & 3], tap_of_g(G)))
    out = b''
    for t in range((w.shape[0] + 15) // 16):
        for rd in range(rounds):
            if ks == 1:       # lane group g = an entry pair of the round
                out += block(t, lambda g, h: rd * 8 + g * 2 + h, lambda g: 0)
                continue
            for s in range(2):      # lane group g = a tap, the round's two entries
                out += block(t, lambda g, h: rd * 2 + h, lambda g: np.array(TAP3[s])[g])
            if rd % 4 == 3 or rd == rounds - 1:      # lane group g = round 4q + g of the group of four, tap (2, 2)
                q = rd // 4
                out += block(t, lambda g, h: np.where(4 * q + g < rounds, (4 * q + g) * 2 + h, len(ent) - 1), lambda g: 8)
    return out, rounds


def ref_fold(w, front, slice_ch, tiles, chunks):
    """R's input channel at K position e of lane group g: chunk 0 = channel e & 3 of group entry 2g + e / 4 of R's other channels, chunk 1 =
    cout 4g + (e & 3) of the producer's cout tile e / 4, chunk 2 = cout 4g + e of its third tile at e < 4, nothing above"""
    c0 = 4 * (2 * G + E8 // 4) + (E8 & 3)
    c1 = 16 * (E8 // 4) + 4 * G + (E8 & 3)
    c2 = 32 + 4 * G + E8
    ci = [np.where(c0 < front, c0, -1), np.where(c1 < slice_ch, front + c1, -1), np.where((E8 < 4) & (c2 < slice_ch), front + c2, -1)]
    return b''.join(pair_blocks(gather(w, t * 16 + N, ci[chunk], 0)) for t in range(tiles) for chunk in range(chunks))


def ref_pair_p(w, r):
    ent = entries([r])
    rounds = (len(ent) + 1) // 2
    ent = np.concatenate([ent, np.full((1, 4), -1)])
    two, nine = b'', b''
    lane4, e4 = np.ogrid[:64, :4]
    for t in range((w.shape[0] + 15) // 16):
        for rd in range(rounds):
            for s in range(2):
                two += pair_blocks(gather(w, t * 16 + N, ent[rd * 2 + E8 // 4, E8 & 3], np.array(TAP3[s])[G]))
            g = lane4 >> 4      # lane groups 0 / 1 = the round's first / second entry, groups 2 and 3 zero
            nine += pair_blocks(gather(w, t * 16 + (lane4 & 15), np.where(g < 2, ent[np.minimum(rd * 2 + g, len(ent) - 1), e4], -1), 8))
    return two, nine, rounds, len(ent) - 1


def packed(layout, w, ks, ranges, stride=1, pad=0, rem=0, tiles=0, chunks=0, short=0):
    """the bytes the layout's writer produced, through a buffer of the size function's floats + 64 sentinels; `short`: the call is told
    of that many floats fewer than the layout has and must refuse without writing (returns None)"""
    L = pflib.load()
    cout, cin, _ = w.shape
    choff = np.array([r[0] for r in ranges], dtype=np.int32)
    ch = np.array([r[1] for r in ranges], dtype=np.int32)
    w = np.ascontiguousarray(w)
    args = (layout, ks, stride, cin, cout, len(ranges), choff.ctypes.data, ch.ctypes.data, pad, rem, tiles, chunks, w.ctypes.data)
    n = ctypes.c_size_t()
    assert L.pf_debug_pack_conv(*args, None, 0, ctypes.byref(n)) == -1 and n.value > 0, L.pf_last_error()   # (PF_EINVAL for no room, but the size)
    buf = np.full(n.value + 64, FILL, dtype=np.uint32)
    rc = L.pf_debug_pack_conv(*args, buf.ctypes.data, n.value - short, ctypes.byref(n))
    if short:
        assert rc == -1 and b'room for' in L.pf_last_error() and (buf == FILL).all()
        return None
    assert rc == 0, L.pf_last_error()
    assert buf.size == n.value + 64 and (buf[n.value:] == FILL).all(), 'the writer ran past what its size function answers'
    body = buf[:n.value]
    left = body.view(np.uint16) == FILL & 0xffff if layout >= SPLIT else body == FILL      # (fp16 pairs: neither half of a float)
    assert not left.any(), 'floats the writer left unwritten'
    return body.tobytes()


SRC = [(0, 10), (0, 7)]       # channel counts that are no multiple of any chunk size: padding falls between the sources


@pytest.mark.parametrize('cout', COUTS)
@pytest.mark.parametrize('ks,stride', [(1, 1), (3, 1), (3, 2)])
def test_generic_and_tiled(ks, stride, cout):
    w = weights(cout, 17, ks)
    assert packed(GENERIC, w, ks, SRC, stride=stride) == ref_generic(w, ks, stride)
    kc = 16 if ks == 1 else (4 if stride == 2 else 8)      # dma_kc
    assert packed(TILED, w, ks, SRC, stride=stride) == ref_tiled(w, [10, 7], kc)


@pytest.mark.parametrize('cout,rem', [(c, r) for c in COUTS for r in (1, 2, 3, 5, 8) if r <= c])      # (the last rem of the conv's couts)
def test_rem(cout, rem):
    w = weights(cout, 17, 3)
    got = packed(REM, w, 3, SRC, rem=rem)
    assert got == ref_rem(w, [10, 7], 8, rem)
    assert len(got) == 4 * (2 + 1) * 2 * 9 * {1: 2, 2: 2, 3: 4, 5: 8, 8: 8}[rem] * 4      # chunks of 8; the rv = 2 form, one group, two groups


@pytest.mark.parametrize('cout', COUTS)
@pytest.mark.parametrize('ks,want_nr', [(1, 0), (3, 2)])
def test_wave(ks, want_nr, cout):
    w = weights(cout, 17, ks)
    ref, nr = ref_wave(w, [10, 7], ks)
    assert nr == want_nr      # an empty and a non-empty remainder group
    assert packed(WAVE, w, ks, SRC) == ref


@pytest.mark.parametrize('cout', COUTS)
def test_split(cout):
    w = weights(cout, 17, 3)
    assert packed(SPLIT, w, 3, SRC) == ref_split(w, [10, 7])


@pytest.mark.parametrize('cout', COUTS)
@pytest.mark.parametrize('src_ch', [(10, 7), (40, 7)])      # (a source of more than one chunk of 32)
def test_split1(src_ch, cout):
    w = weights(cout, sum(src_ch), 1)
    assert packed(SPLIT1, w, 1, [(0, c) for c in src_ch]) == ref_split1(w, src_ch)


A, B, C = (2, 10), (0, 18), (4, 22)      # ranges at even offsets that are no multiple of 4: 3, 5 and 6 group entries


# rounds: the collected-tap block alone, after a full group of four, after a short last group (1 and 3 rounds)
@pytest.mark.parametrize('cout', COUTS)
@pytest.mark.parametrize('ks,ranges,pad,want_rounds', [(3, [(2, 6)], 0, 1), (3, [A, B], 0, 4), (3, [A, B], 1, 5), (3, [A, B, C], 0, 7),
                                                      (3, [A, B, C], 1, 8), (1, [A, B], 1, 2), (1, [A, B], 0, 1)])
def test_s4(ks, ranges, pad, want_rounds, cout):
    w = weights(cout, sum(r[1] for r in ranges), ks)
    ref, rounds = ref_s4(w, ks, ranges, pad)
    assert rounds == want_rounds
    assert packed(S4, w, ks, ranges, pad=pad) == ref


@pytest.mark.parametrize('cout', COUTS)
@pytest.mark.parametrize('chunks,slice_ch', [(2, 20), (3, 40)])
def test_fold(chunks, slice_ch, cout):
    front = 10      # R's range starts on a group (channel 4), the slice at channel 14 = 2 (mod 4)
    w = weights(cout, front + slice_ch, 1)
    assert packed(FOLD, w, 1, [(4, front), (4 + front, slice_ch)], tiles=2, chunks=chunks) == ref_fold(w, front, slice_ch, 2, chunks)


@pytest.mark.parametrize('cout', COUTS)
def test_pair_p(cout):
    w = weights(cout, 10, 3)
    two, nine, rounds, n_ent = ref_pair_p(w, A)
    assert (rounds, n_ent) == (2, 3)      # an odd entry count: the last round's second entry is absent
    assert packed(PAIR_TWO, w, 3, [A]) == two
    got = packed(PAIR_NINE, w, 3, [A])
    assert got == nine
    lanes = np.frombuffer(got, dtype=np.uint16).reshape(-1, 2, 64, 4)
    assert not lanes[:, :, 32:].any() and lanes[:, :, :32].any()      # lane groups 2 and 3 are zero


def test_refusals():
    """too little room (nothing is written) and arguments no layout has"""
    w = weights(5, 17, 3)
    for layout, ks in ((GENERIC, 3), (TILED, 3), (WAVE, 3), (SPLIT, 3), (S4, 3)):
        packed(layout, w, ks, SRC, short=1)
    packed(REM, w, 3, SRC, rem=3, short=1)
    packed(PAIR_NINE, weights(5, 10, 3), 3, [A], short=1)
    packed(FOLD, weights(5, 30, 1), 1, [(4, 10), (14, 20)], tiles=2, chunks=2, short=1)
    L = pflib.load()
    n = ctypes.c_size_t()
    choff, ch = (ctypes.c_int * 4)(0, 0, 0, 0), (ctypes.c_int * 4)(10, 7, 0, 0)
    bad = [(10, 3, 1, 17, 5, 2, 0, 0), (SPLIT, 1, 1, 17, 5, 2, 0, 0), (SPLIT1, 3, 1, 17, 5, 2, 0, 0), (TILED, 3, 1, 18, 5, 2, 0, 0),
           (REM, 3, 1, 17, 5, 2, 0, 6), (REM, 3, 1, 17, 5, 2, 0, 0), (PAIR_TWO, 3, 1, 17, 5, 2, 0, 0), (TILED, 2, 1, 17, 5, 2, 0, 0), (TILED, 3, 1, 17, 5, 5, 0, 0)]
    for layout, ks, stride, cin, cout, n_src, pad, rem in bad:
        assert L.pf_debug_pack_conv(layout, ks, stride, cin, cout, n_src, choff, ch, pad, rem, 0, 0, w.ctypes.data, None, 0, ctypes.byref(n)) == -1
        assert b'pf_debug_pack_conv' in L.pf_last_error()
