"""The range tables of a convolution launch (csrc/conv_ranges.cpp, through pf_debug_conv_ranges): host code only, no GPU.

The references below restate the loops the schedules and packers carried themselves at 56bf59a, before the tables moved into one
module: conv_step / conv_args (src_cstart), the `use` lambda and the `dma` lambda (src_chunk0, chunk_begin / chunk_end), steps 4 and 5
of build_schedule (the packed-pair tables of a plain launch, of the conv_pair consumer and of the add launch) and pack_pair / pack_share
(the order and the weight-numbering start of each range).  They run on all cases of a call at once, arrays of [field or range][cases],
one loop turn per range as the originals.

Two fields no kernel of those launches reads are defined by the module where the schedule used to leave what the plain launch had put
there: ConvArgs::src_cstart of the pair and add launches (now the prefix sums of the launch's own ranges) and chunk_begin / chunk_end of
the pair launch (now 0 and its rounds).
"""
import itertools

import numpy as np
import pytest

from panoptic_forecasting_amd import hardnet_arch
from panoptic_forecasting_amd import lib as pflib

MAX_SRC = 4
PLAIN, PAIR, ADD = 0, 1, 2
N, COUNT, ORDER, CSTART, WSTART, CHUNK0, C4, G0, GN, ENT0, CHUNK_BEGIN, CHUNK_END = (
    slice(0, 1), slice(1, 2), slice(2, 6), slice(6, 11), slice(11, 15), slice(15, 20), slice(20, 24), slice(24, 28), slice(28, 32),
    slice(32, 37), slice(37, 38), slice(38, 39))


def tables(form, ks, kc, pad, n_src, choff, ch, ctotal, begin=-1, end=-1):
    """[39][cases] of pf_debug_conv_ranges for [cases][4] ranges"""
    choff, ch, ctotal = (np.ascontiguousarray(x, dtype=np.int32) for x in (choff, ch, ctotal))
    out = np.full((choff.shape[0], 39), -7, dtype=np.int32)
    pflib.check(pflib.load().pf_debug_conv_ranges(form, ks, kc, pad, n_src, choff.shape[0], choff.ctypes.data, ch.ctypes.data, ctotal.ctypes.data,
                                                  begin, end, out.ctypes.data, out.size), 'pf_debug_conv_ranges')
    return np.ascontiguousarray(out.T)


def blank(cases):
    return np.zeros((39, cases), dtype=np.int32)


def ref_cstart(out, n, ch):
    """conv_step / conv_args: prefix sums of the range lengths, the tail = their total"""
    c0 = np.zeros(ch.shape[1], dtype=np.int32)
    for j in range(n):
        out[CSTART][j] = c0
        c0 = c0 + ch[j]
    for j in range(n, MAX_SRC + 1):
        out[CSTART][j] = c0


def ref_chunks(n, ch, kc, begin, end):
    """the `use` lambda of build_schedule (and the `dma` lambda of build_train_schedule): chunks of kc channels"""
    out = blank(ch.shape[1])
    out[N] = n
    out[ORDER][:n] = np.arange(n)[:, None]
    ref_cstart(out, n, ch)
    out[WSTART][:n] = out[CSTART][:n]
    c0 = out[CHUNK0]
    for j in range(MAX_SRC):
        c0[j + 1] = c0[j] + ((ch[j] + kc - 1) // kc if j < n else 0)
    out[CHUNK_BEGIN] = c0[begin:begin + 1]
    out[CHUNK_END] = c0[end:end + 1]
    out[COUNT] = c0[n:n + 1]          # dma_chunks / wave_chunks / split_chunks / split1_chunks: sum over ranges of ceil(ch / kc)
    assert (out[COUNT][0] == sum((ch[j] + kc - 1) // kc for j in range(n))).all()
    return out


def ref_s4_plain(n, choff, ch, ctotal, ks, pad, begin, end):
    """step 4 of build_schedule (and the conv_s4 branch of build_train_schedule): the packed-pair tables of the op's ranges as they are"""
    out = blank(ch.shape[1])
    out[N] = n
    out[ORDER][:n] = np.arange(n)[:, None]
    ref_cstart(out, n, ch)
    out[WSTART][:n] = out[CSTART][:n]
    per = 2 if ks == 3 else 8
    e = np.zeros(ch.shape[1], dtype=np.int32)
    for j in range(n):
        ch0, chn = choff[j], out[CSTART][j + 1] - out[CSTART][j]
        out[C4][j] = (ctotal[j] + 3) // 4
        out[G0][j] = ch0 // 4
        out[GN][j] = (ch0 + chn + 3) // 4 - ch0 // 4
        out[ENT0][j] = e
        e = e + ((out[GN][j] + per - 1) // per * per if pad else out[GN][j])
    for j in range(n, MAX_SRC + 1):
        out[ENT0][j] = e
    out[CHUNK_BEGIN] = out[ENT0][begin:begin + 1] // per
    out[CHUNK_END] = (out[ENT0][end:end + 1] + per - 1) // per
    out[COUNT][0] = (e + per - 1) // per       # s4_rounds
    return out


def ref_s4_pair(n, choff, ch, ctotal):
    """step 5 of build_schedule, the conv_pair launch, and pack_pair: [S, others.., P], P at channel 0, every range padded to whole rounds"""
    out = blank(ch.shape[1])
    out[N] = n
    c0s = np.concatenate([np.zeros((1, ch.shape[1]), dtype=np.int32), np.cumsum(ch[:n], axis=0, dtype=np.int32)])
    e = np.zeros(ch.shape[1], dtype=np.int32)
    tot = np.zeros(ch.shape[1], dtype=np.int32)
    for j in range(n):
        sj = (j + 1) % n
        is_p = j == n - 1
        out[ORDER][j] = sj
        out[WSTART][j] = c0s[sj]                      # pack_pair: cstart[j] = c0s[sj]
        out[CSTART][j] = tot                             # (ConvArgs::src_cstart: prefix sums in the launch's order)
        tot = tot + ch[sj]
        out[C4][j] = (ctotal[sj] + 3) // 4
        out[G0][j] = 0 if is_p else choff[sj] // 4
        out[GN][j] = (ch[sj] + 3) // 4 if is_p else (choff[sj] + ch[sj] + 3) // 4 - choff[sj] // 4
        out[ENT0][j] = e
        e = e + (out[GN][j] + 1) // 2 * 2
    for j in range(n, MAX_SRC + 1):
        out[ENT0][j] = e
        out[CSTART][j] = tot
    out[COUNT][0] = (e + 1) // 2                         # pair_rounds = s4_rounds(rg, n, 3, 1)
    out[CHUNK_END] = out[COUNT]                          # (conv_pair.hip reads neither chunk_begin nor chunk_end; the schedule left 0, 0)
    return out


def ref_s4_add(n, choff, ch, ctotal):
    """step 5 of build_schedule, the add launch, and pack_share: the consumer without its range 1, nothing padded"""
    out = blank(ch.shape[1])
    out[N] = n - 1
    c0 = np.zeros(ch.shape[1], dtype=np.int32)
    tot = np.zeros(ch.shape[1], dtype=np.int32)
    e = np.zeros(ch.shape[1], dtype=np.int32)
    k = 0
    for j in range(n):
        if j != 1:
            out[ORDER][k] = j
            out[WSTART][k] = c0                          # pack_share: cstart[k++] = c0
            out[CSTART][k] = tot
            tot = tot + ch[j]
            out[C4][k] = (ctotal[j] + 3) // 4
            out[G0][k] = choff[j] // 4
            out[GN][k] = (choff[j] + ch[j] + 3) // 4 - choff[j] // 4
            out[ENT0][k] = e
            e = e + out[GN][k]
            k += 1
        c0 = c0 + ch[j]
    for j in range(n - 1, MAX_SRC + 1):
        out[ENT0][j] = e
        out[CSTART][j] = tot
    out[COUNT][0] = (e + 1) // 2                         # share_b_rounds = s4_rounds(rg, n - 1, 3, 0)
    out[CHUNK_END] = out[COUNT]                          # chunk_begin = 0, chunk_end = nchunks
    return out


def check_all_forms(n, choff, ch, ctotal):
    """every form a conv of n ranges can take; returns the number of launches compared"""
    seen = 0
    rows = choff, ch, ctotal
    choff, ch, ctotal = (np.ascontiguousarray(x.T, dtype=np.int32) for x in rows)      # [range][cases] for the references
    halves = [(0, n)] + ([(0, 1), (1, 2)] if n == 2 else [])       # a commuted upsample + 1x1 runs its two ranges one at a time
    for kc in (4, 8, 16, 32):
        for begin, end in halves:
            got = tables(PLAIN, 3, kc, 0, n, *rows, begin, end)
            assert np.array_equal(got, ref_chunks(n, ch, kc, begin, end)), (kc, begin, end)
            assert np.array_equal(got[COUNT], got[CHUNK0][n:n + 1])       # what the plan stores as tiled / split / wave_chunks
            seen += got.shape[1]
    for ks, pad in itertools.product((1, 3), (0, 1)):
        for begin, end in (halves if pad else halves[:1]):
            got = tables(PLAIN, ks, 0, pad, n, *rows, begin, end)
            assert np.array_equal(got, ref_s4_plain(n, choff, ch, ctotal, ks, pad, begin, end)), (ks, pad, begin, end)
            per = 2 if ks == 3 else 8
            assert np.array_equal(got[COUNT], (got[ENT0][n:n + 1] + per - 1) // per)   # s4_rounds
            seen += got.shape[1]
    if n >= 2:
        got = tables(PAIR, 3, 0, 1, n, *rows)
        assert np.array_equal(got, ref_s4_pair(n, choff, ch, ctotal))
        assert np.array_equal(got[COUNT], got[ENT0][n:n + 1] // 2)                     # pair_rounds (every range padded: even)
        got = tables(ADD, 3, 0, 0, n, *rows)
        assert np.array_equal(got, ref_s4_add(n, choff, ch, ctotal))
        assert np.array_equal(got[COUNT], (got[ENT0][n - 1:n] + 1) // 2)               # share_b_rounds
        seen += 2 * got.shape[1]
    return seen


def test_every_convolution_of_the_default_network():
    spec = hardnet_arch.Spec()
    by_n = {}
    for op in spec.conv_ops():
        row = [[s.choff for s in op.srcs], [s.ch for s in op.srcs], [spec.tensors[s.tensor].channels for s in op.srcs]]
        by_n.setdefault(len(op.srcs), []).append([r + [0] * (MAX_SRC - len(r)) for r in row])
    assert set(by_n) == {1, 2, 3, 4}
    for n, rows in by_n.items():
        a = np.array(rows, dtype=np.int32)
        assert check_all_forms(n, a[:, 0], a[:, 1], a[:, 2]) > 0


@pytest.mark.parametrize('n', [1, 2, 3, 4])
def test_all_combinations_of_ranges(n):
    """ranges that begin or end inside a group of four and inside a chunk"""
    one = np.array(list(itertools.product((0, 2, 4, 6, 10), (1, 2, 3, 4, 5, 8, 9, 17))), dtype=np.int32)      # (choff, ch)
    idx = np.stack(np.meshgrid(*[np.arange(len(one))] * n, indexing='ij'), axis=-1).reshape(-1, n)
    assert idx.shape[0] == 40 ** n
    for part in np.array_split(idx, max(1, idx.shape[0] // 16384)):
        choff = np.zeros((part.shape[0], MAX_SRC), dtype=np.int32)
        ch = np.zeros_like(choff)
        choff[:, :n], ch[:, :n] = one[part, 0], one[part, 1]
        ctotal = choff + ch + np.arange(MAX_SRC)        # tensors with 0..3 channels behind the range: whole and partial last groups
        check_all_forms(n, choff, ch, ctotal)
