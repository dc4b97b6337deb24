// The weight layouts of the convolution kernels (conv_pack.h): OIHW fp32 -> what each kernel family streams.  Host code only: plain
// loops over float arrays, one writer per layout with its size function beside it, the layout's index formula above the writer.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "conv_ranges.h"
#include "conv_s4.h"

namespace pf {

namespace {

// the conv's weights, zero outside it: at(co, ci, tap) for any co, ci (ci = -1: a padding channel)
struct Oihw {
    const float *w;
    int cin, cout, ks2;
    float at(int co, int ci, int tap) const { return (co < cout && ci >= 0 && ci < cin) ? w[((size_t)co * cin + ci) * ks2 + tap] : 0.f; }
};

// one chunk of kc input channels of the K order "ranges in order, each padded to whole chunks": its channel k is the conv's ci(k)
struct Chunk {
    int c0, n;   // conv input channels [c0, c0 + n), padding behind them
    int ci(int k) const { return k < n ? c0 + k : -1; }
};
template <typename F>
void for_chunks(const int *src_ch, int n_src, int kc, F f) {
    int c0 = 0;
    for (int j = 0; j < n_src; c0 += src_ch[j++])
        for (int lc = 0; lc * kc < src_ch[j]; ++lc) f(Chunk{c0 + lc * kc, std::min(kc, src_ch[j] - lc * kc)});
}

// one fp16-pair block [term 2: hi, mid][lane 64][E fp16] of value(lane, e) at o; returns the block's end
template <int E, typename F>
unsigned short *put_pair_block(unsigned short *o, F value) {
    for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < E; ++e) {
            const float v = value(lane, e);
            const unsigned short hi = split_host_f16(v);
            o[lane * E + e] = hi;
            o[(64 + lane) * E + e] = split_host_f16(v - split_host_f32(hi));
        }
    return o + 2 * 64 * E;
}

// ky * 3 + kx of (instr, lane group) of a 3x3 packed-pair round: see the kernel's aoff (conv_s4_kernel.inc); the ninth tap (2,2) is
// collected apart
constexpr int kTap3[2][4] = {{0, 1, 3, 4}, {6, 7, 2, 5}};

inline int cout_tiles(int cout) { return (cout + 15) / 16; }

}  // namespace

// ---- host halves of the operand split (conv_mfma.h)
unsigned short split_host_f16(float x) {
    unsigned u;
    memcpy(&u, &x, 4);
    const unsigned short sign = (unsigned short)((u >> 16) & 0x8000u);
    u &= 0x7fffffffu;
    if (u >= 0x7f800000u) return (unsigned short)(sign | (u > 0x7f800000u ? 0x7e00u : 0x7c00u));   // nan / inf
    if (u >= 0x477ff000u) return (unsigned short)(sign | 0x7c00u);                                  // >= 65520 rounds to inf
    if (u < 0x38800000u) {   // below 2^-14: a multiple of the subnormal step 2^-24 (1024 steps = the smallest normal: same bits)
        float f;
        memcpy(&f, &u, 4);
        return (unsigned short)(sign | (unsigned)nearbyintf(f * 16777216.0f));   // default rounding mode: nearest even
    }
    u -= 0x38000000u;                        // exponent bias 127 -> 15
    u += 0xfffu + ((u >> 13) & 1u);          // nearest even on the 13 dropped bits (a carry moves into the exponent)
    return (unsigned short)(sign | (u >> 13));
}
float split_host_f32(unsigned short h) {
    const unsigned sign = (unsigned)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    float f;
    if (e == 0) {
        f = (float)m * (1.0f / 16777216.0f);
        unsigned u;
        memcpy(&u, &f, 4);
        u |= sign;
        memcpy(&f, &u, 4);
        return f;
    }
    const unsigned u = sign | (e == 31 ? 0x7f800000u | (m << 13) : ((e + 112u) << 23) | (m << 13));
    memcpy(&f, &u, 4);
    return f;
}
float split_weight_scale(const float *w, size_t n) {
    float mx = 0.f;
    for (size_t i = 0; i < n; ++i) mx = fmaxf(mx, fabsf(w[i]));
    if (!(mx > 0.f) || !std::isfinite(mx)) return 1.0f;
    int e;
    frexpf(mx, &e);                          // mx = f * 2^e, f in [0.5, 1)
    return ldexpf(1.0f, 15 - e);             // mx * 2^(15 - e) in [2^14, 2^15)
}

// ------------------------------------------------------------------------------------------------ fp32 layouts
// generic kernel: [cout_block][chunk][kgroup][tap][nt][64 lanes] with
//   value = W[(cb*nt+t)*16 + (lane&15)][chunk*kc + kg*4 + (lane>>4)][tap]  (0 outside Cin/Cout)
size_t ConvTiling::packed_floats() const { return (size_t)cout_blocks * nchunks * (kc / 4) * ks * ks * nt * 64; }
void pack_conv_weights(const float *w, int cin, int cout, const ConvTiling &t, float *out) {
    const Oihw W{w, cin, cout, t.ks * t.ks};
    for (int cb = 0; cb < t.cout_blocks; ++cb)
        for (int ch = 0; ch < t.nchunks; ++ch)
            for (int kg = 0; kg < t.kc / 4; ++kg)
                for (int tap = 0; tap < W.ks2; ++tap)
                    for (int n = 0; n < t.nt; ++n)
                        for (int lane = 0; lane < 64; ++lane) *out++ = W.at((cb * t.nt + n) * 16 + (lane & 15), ch * t.kc + kg * 4 + (lane >> 4), tap);
}

// per-tile packing: [cout tile][chunk][kgroup][tap][64 lanes]; K order = the input ranges in order, each padded to
// whole chunks (zero weights), so a chunk never straddles two source tensors
size_t tiled_packed_floats(const int *src_ch, int n_src, int cout, int ks, int stride) {
    return (size_t)cout_tiles(cout) * range_chunks(src_ch, n_src, dma_kc(ks, stride)) * (dma_kc(ks, stride) / 4) * ks * ks * 64;
}
void pack_conv_weights_tiled(const float *w, int cin, int cout, int ks, int kc, const int *src_ch, int n_src, float *out) {
    const Oihw W{w, cin, cout, ks * ks};
    for (int t = 0; t < cout_tiles(cout); ++t)
        for_chunks(src_ch, n_src, kc, [&](Chunk ch) {
            for (int kg = 0; kg < kc / 4; ++kg)
                for (int tap = 0; tap < W.ks2; ++tap)
                    for (int lane = 0; lane < 64; ++lane) *out++ = W.at(t * 16 + (lane & 15), ch.ci(kg * 4 + (lane >> 4)), tap);
        });
}

// [chunk][kgroup][tap][rv/4][4 input channels][4 couts] (rv = 2: [chunk][kgroup][tap][2 couts][4 input channels]):
// the last `rem` output channels, zero padded to rv = dma_rem_rv(rem)
size_t rem_packed_floats(const int *src_ch, int n_src, int rem, int ks, int kc) {
    return (size_t)range_chunks(src_ch, n_src, kc) * (kc / 4) * ks * ks * dma_rem_rv(rem) * 4;
}
void pack_conv_weights_rem(const float *w, int cin, int cout, int rem, int ks, int kc, const int *src_ch, int n_src, float *out) {
    const Oihw W{w, cin, cout, ks * ks};
    const int rv = dma_rem_rv(rem), co0 = cout - rem;   // (rows past rem are past cout: zero)
    for_chunks(src_ch, n_src, kc, [&](Chunk ch) {
        for (int kg = 0; kg < kc / 4; ++kg)
            for (int tap = 0; tap < W.ks2; ++tap) {
                if (rv == 2) {   // [cout][4 input channels]: read as two uniform 16-B rows
                    for (int r = 0; r < 2; ++r)
                        for (int c = 0; c < 4; ++c) *out++ = W.at(co0 + r, ch.ci(kg * 4 + c), tap);
                    continue;
                }
                for (int g = 0; g < rv / 4; ++g)
                    for (int c = 0; c < 4; ++c)
                        for (int q = 0; q < 4; ++q) *out++ = W.at(co0 + g * 4 + q, ch.ci(kg * 4 + c), tap);
            }
    });
}

// fragment-order packing for direct L2 -> VGPR loads, per (cout tile, chunk): [quad][64 lanes][4] then the
// remainder [64 lanes][NR];  value idx = q*4+e (or 4*NQ+e) -> (kg, tap) = (idx / ks2, idx % ks2):
//   W[t*16 + (lane&15)][first channel of the chunk + kg*4 + (lane>>4)][tap]
// K order: the input ranges in order, each padded to whole chunks (zeros), so a chunk lies inside one tensor.
size_t wave_packed_floats(const int *src_ch, int n_src, int cout, int ks) {
    const int kc = wave_kc(ks), nv = (kc / 4) * ks * ks;
    return (size_t)cout_tiles(cout) * range_chunks(src_ch, n_src, kc) * ((nv / 4) * 256 + (nv % 4) * 64);
}
void pack_conv_weights_wave(const float *w, int cin, int cout, int ks, const int *src_ch, int n_src, float *out) {
    const Oihw W{w, cin, cout, ks * ks};
    const int kc = wave_kc(ks), nv = (kc / 4) * W.ks2, nq = nv / 4, nr = nv % 4;
    for (int t = 0; t < cout_tiles(cout); ++t)
        for_chunks(src_ch, n_src, kc, [&](Chunk ch) {
            auto val = [&](int idx, int lane) { return W.at(t * 16 + (lane & 15), ch.ci(idx / W.ks2 * 4 + (lane >> 4)), idx % W.ks2); };
            for (int q = 0; q < nq; ++q)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 4; ++e) *out++ = val(q * 4 + e, lane);
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < nr; ++e) *out++ = val(nq * 4 + e, lane);
        });
}

// ------------------------------------------------------------------------------------------------ fp16-pair layouts
// conv_split 3x3, bytes as floats (the weight arena is a float array): [tile][chunk][step 3][term 2][lane 64][8 fp16] = 16 B per lane;
// lane = (cout n = lane & 15, tap 4 * step + (lane >> 4); taps past the ninth are zero), the lane's 8 values = the chunk's 8 channels
size_t split_packed_floats(const int *src_ch, int n_src, int cout) {
    return (size_t)cout_tiles(cout) * range_chunks(src_ch, n_src, 8) * 3 * 2 * 64 * 4;
}
void pack_conv_weights_split(const float *w, int cin, int cout, const int *src_ch, int n_src, float *out_f) {
    const Oihw W{w, cin, cout, 9};
    unsigned short *out = reinterpret_cast<unsigned short *>(out_f);
    for (int t = 0; t < cout_tiles(cout); ++t)
        for_chunks(src_ch, n_src, 8, [&](Chunk ch) {
            for (int s = 0; s < 3; ++s)
                out = put_pair_block<8>(out, [&](int lane, int e) {
                    const int tap = 4 * s + (lane >> 4);
                    return tap < 9 ? W.at(t * 16 + (lane & 15), ch.ci(e), tap) : 0.f;
                });
        });
}

// conv_split 1x1, bytes as floats: [tile][chunk of 32 ch][term 2][lane 64][8 fp16]; lane = (cout n = lane & 15, k-group lane >> 4)
size_t split1_packed_floats(const int *src_ch, int n_src, int cout) {
    return (size_t)cout_tiles(cout) * range_chunks(src_ch, n_src, 32) * 2 * 64 * 4;
}
void pack_conv_weights_split1(const float *w, int cin, int cout, const int *src_ch, int n_src, float *out_f) {
    const Oihw W{w, cin, cout, 1};
    unsigned short *out = reinterpret_cast<unsigned short *>(out_f);
    for (int t = 0; t < cout_tiles(cout); ++t)
        for_chunks(src_ch, n_src, 32, [&](Chunk ch) {
            out = put_pair_block<8>(out, [&](int lane, int e) { return W.at(t * 16 + (lane & 15), ch.ci((lane >> 4) * 8 + e), 0); });
        });
}

// Blocks of [term 2][lane 64][8 fp16]; lane = (cout n = lane & 15, lane group g = lane >> 4), the lane's 8 values = 4 channels
// of two group entries.  1x1: [tile][round], g = entry pair of the round.  3x3: [tile][per round: instr 0, instr 1, and after
// every 4th (and the last) round the collected-tap block]; instr blocks: g = tap, entries of the round; collected block:
// g = round 4q + g of its group of four, tap (2,2)
size_t s4_packed_floats(const KOrder &k, int cout, int ks, int pad_sources) {
    const int rounds = s4_rounds(k, ks, pad_sources);
    return (size_t)cout_tiles(cout) * (ks == 3 ? s4_blocks_total(rounds) : rounds) * 2 * 64 * 4;
}
void pack_conv_weights_s4(const float *w, int cin, int cout, int ks, const KOrder &k, int pad_sources, float *out_f) {
    const Oihw W{w, cin, cout, ks * ks};
    unsigned short *out = reinterpret_cast<unsigned short *>(out_f);
    // entry -> (first conv input channel of the group's channel 0, may be negative; valid channel window)
    struct Entry { int c0, lo, hi; };
    std::vector<Entry> ent;
    const int per = s4_per_round(ks);
    for (int j = 0; j < k.n; ++j) {
        const KRange &r = k.r[j];
        const int g0 = r.choff / 4;
        for (int g = g0; g < g0 + s4_range_groups(r.choff, r.ch); ++g) ent.push_back(Entry{r.cstart + 4 * g - r.choff, r.cstart, r.cstart + r.ch});
        while (pad_sources && ent.size() % per != 0) ent.push_back(Entry{0, 0, 0});   // padding entry: no valid channel
    }
    const int n_ent = (int)ent.size(), rounds = (n_ent + per - 1) / per;
    // one block: value of (lane, e) = weight of cout (t, lane & 15), entry ent_of(lane >> 4, e / 4), channel e & 3, tap tap_of(lane >> 4)
    auto block = [&](int t, auto ent_of, auto tap_of) {
        out = put_pair_block<8>(out, [&](int lane, int e) {
            const int g = lane >> 4, en = ent_of(g, e / 4);
            if (en < 0 || en >= n_ent) return 0.f;
            const int ci = ent[en].c0 + (e & 3);
            return W.at(t * 16 + (lane & 15), ci >= ent[en].lo && ci < ent[en].hi ? ci : -1, tap_of(g));
        });
    };
    for (int t = 0; t < cout_tiles(cout); ++t)
        for (int rd = 0; rd < rounds; ++rd) {
            if (ks == 1) {
                block(t, [&](int g, int h) { return rd * 8 + g * 2 + h; }, [](int) { return 0; });
                continue;
            }
            for (int s = 0; s < 2; ++s) block(t, [&](int, int h) { return rd * 2 + h; }, [&](int g) { return kTap3[s][g]; });
            if ((rd & 3) == 3 || rd == rounds - 1) {
                const int q = rd / 4;
                block(t, [&](int g, int h) { return 4 * q + g < rounds ? (4 * q + g) * 2 + h : -1; }, [](int) { return 8; });
            }
        }
}

// the fold forms' second conv R: [cout tile ntiles][chunk (2, or 3 for a producer of three cout tiles)][term 2][lane 64][8 fp16], lane = (cout lane & 15 of the tile, lane group g),
// value e = R's weight of the input channel tail_channel(k, chunk, g, e) (conv_ranges.cpp), zero where there is none and past R's couts
// (floats: fold_packed_floats, conv_mfma.h)
void pack_conv_weights_fold(const float *w, int cin, int cout, const KOrder &k, int ntiles, float *out_f, int chunks) {
    const Oihw W{w, cin, cout, 1};
    unsigned short *out = reinterpret_cast<unsigned short *>(out_f);
    for (int t = 0; t < ntiles; ++t)
        for (int chunk = 0; chunk < chunks; ++chunk)
            out = put_pair_block<8>(out, [&](int lane, int e) { return W.at(t * 16 + (lane & 15), tail_channel(k, chunk, lane >> 4, e), 0); });
}

// conv_pair: P's weights.  `two`: blocks of [term 2][lane 64][8 fp16] as in pack_conv_weights_s4 (lane = cout n = lane & 15,
// lane group g = tap of instr 0 / 1, the lane's 8 values = 4 channels of the round's two entries), two per round and tile, no
// collected-tap blocks.  `nine`: per round and tile [term 2][lane 64][4 fp16]: lane group 0 / 1 = tap (2,2) of the round's first /
// second entry, groups 2 and 3 zero (K = 16 instruction)
static int pair_p_rounds(const S4Range &r) { return (s4_range_groups(r.choff, r.ch) + 1) / 2; }
size_t pair_p_two_floats(const S4Range &r, int cout) { return (size_t)cout_tiles(cout) * pair_p_rounds(r) * 2 * (2 * 64 * 4); }
size_t pair_p_nine_floats(const S4Range &r, int cout) { return (size_t)cout_tiles(cout) * pair_p_rounds(r) * (2 * 64 * 2); }
void pack_conv_weights_pair_p(const float *w, int cin, int cout, const S4Range &r, float *two_f, float *nine_f) {
    const Oihw W{w, cin, cout, 9};
    unsigned short *two = reinterpret_cast<unsigned short *>(two_f), *nine = reinterpret_cast<unsigned short *>(nine_f);
    const int g0 = r.choff / 4, n_ent = s4_range_groups(r.choff, r.ch);
    // weight of (cout co, entry ent, channel slot e of the group, tap): zero outside the range / the layer
    auto wv = [&](int co, int ent, int e, int tap) {
        const int ci = 4 * (g0 + ent) + e - r.choff;
        return W.at(co, ent < n_ent && ci < r.ch ? ci : -1, tap);
    };
    for (int t = 0; t < cout_tiles(cout); ++t)
        for (int rd = 0; rd < pair_p_rounds(r); ++rd) {
            for (int s = 0; s < 2; ++s)
                two = put_pair_block<8>(two, [&](int lane, int e) { return wv(t * 16 + (lane & 15), rd * 2 + e / 4, e & 3, kTap3[s][lane >> 4]); });
            nine = put_pair_block<4>(nine, [&](int lane, int e) { return (lane >> 4) < 2 ? wv(t * 16 + (lane & 15), rd * 2 + (lane >> 4), e, 8) : 0.f; });
        }
}

}  // namespace pf

// pf_debug_pack_conv (include/pfhip.h documents the layouts and the arguments)
extern "C" int pf_debug_pack_conv(int layout, int ks, int stride, int cin, int cout, int n_src, const int *choff, const int *ch, int pad_sources,
                                  int rem, int tiles, int chunks, const float *w, float *out, size_t cap, size_t *n_floats) {
    using namespace pf;
    enum { GENERIC, TILED, REM, WAVE, SPLIT, SPLIT1, S4, FOLD, PAIR_TWO, PAIR_NINE, N_LAYOUTS };
    if (!choff || !ch || !w || !n_floats || (!out && cap)) return fail(PF_EINVAL, "pf_debug_pack_conv: null argument");
    const int want_ks = (layout == SPLIT || layout == PAIR_TWO || layout == PAIR_NINE) ? 3 : (layout == SPLIT1 || layout == FOLD) ? 1 : ks;
    const int want_src = layout == FOLD ? 2 : (layout == PAIR_TWO || layout == PAIR_NINE) ? 1 : n_src;
    if (layout < 0 || layout >= N_LAYOUTS || (ks != 1 && ks != 3) || ks != want_ks || (stride != 1 && stride != 2) || cout < 1 || n_src < 1 ||
        n_src > kConvMaxSrc || n_src != want_src)
        return fail(PF_EINVAL, "pf_debug_pack_conv: layout %d, ks %d, stride %d, %d couts, %d ranges", layout, ks, stride, cout, n_src);
    BlobSrc src[kConvMaxSrc];
    int total = 0;
    for (int j = 0; j < n_src; ++j) {
        if (choff[j] < 0 || ch[j] < (layout == FOLD ? 0 : 1)) return fail(PF_EINVAL, "pf_debug_pack_conv: range %d = (%d, %d)", j, choff[j], ch[j]);
        src[j] = BlobSrc{(uint32_t)j, (uint32_t)choff[j], (uint32_t)ch[j]};
        total += ch[j];
    }
    if (total != cin) return fail(PF_EINVAL, "pf_debug_pack_conv: the ranges hold %d channels, cin = %d", total, cin);
    if (layout == REM && (rem < 1 || rem > 16 || rem > cout)) return fail(PF_EINVAL, "pf_debug_pack_conv: rem %d of %d couts", rem, cout);
    if (layout == FOLD && (choff[1] != choff[0] + ch[0] || tiles < 1 || chunks < kTailChunks || chunks > kWideChunks))
        return fail(PF_EINVAL, "pf_debug_pack_conv: fold: [R's other channels, the slice behind them], tiles >= 1, 2 or 3 chunks");
    // (the fold forms cut R's single range at the slice: order_tail)
    const KOrder k = layout == FOLD ? order_tail(BlobSrc{0, (uint32_t)choff[0], (uint32_t)cin}, choff[1], ch[1]) : order_plain(src, n_src);
    const S4Range r{choff[0], ch[0]};
    const ConvTiling t = choose_tiling(ks, stride, cin, cout, 0);
    const int kc = dma_kc(ks, stride);
    auto room = [&](size_t n) { *n_floats = n; return cap >= n; };
    bool ok = false;
    switch (layout) {
    case GENERIC: if ((ok = room(t.packed_floats()))) pack_conv_weights(w, cin, cout, t, out); break;
    case TILED: if ((ok = room(tiled_packed_floats(ch, n_src, cout, ks, stride)))) pack_conv_weights_tiled(w, cin, cout, ks, kc, ch, n_src, out); break;
    case REM: if ((ok = room(rem_packed_floats(ch, n_src, rem, ks, kc)))) pack_conv_weights_rem(w, cin, cout, rem, ks, kc, ch, n_src, out); break;
    case WAVE: if ((ok = room(wave_packed_floats(ch, n_src, cout, ks)))) pack_conv_weights_wave(w, cin, cout, ks, ch, n_src, out); break;
    case SPLIT: if ((ok = room(split_packed_floats(ch, n_src, cout)))) pack_conv_weights_split(w, cin, cout, ch, n_src, out); break;
    case SPLIT1: if ((ok = room(split1_packed_floats(ch, n_src, cout)))) pack_conv_weights_split1(w, cin, cout, ch, n_src, out); break;
    case S4: if ((ok = room(s4_packed_floats(k, cout, ks, pad_sources)))) pack_conv_weights_s4(w, cin, cout, ks, k, pad_sources, out); break;
    case FOLD: if ((ok = room(fold_packed_floats(tiles, chunks)))) pack_conv_weights_fold(w, cin, cout, k, tiles, out, chunks); break;
    default: {   // the two streams of conv_pair's producer come from one writer: the other one goes to a scratch buffer
        const size_t n2 = pair_p_two_floats(r, cout), n9 = pair_p_nine_floats(r, cout);
        std::vector<float> other(layout == PAIR_TWO ? n9 : n2);
        if ((ok = room(layout == PAIR_TWO ? n2 : n9))) pack_conv_weights_pair_p(w, cin, cout, r, layout == PAIR_TWO ? out : other.data(), layout == PAIR_TWO ? other.data() : out);
    }
    }
    return ok ? PF_OK : fail(PF_EINVAL, "pf_debug_pack_conv: room for %zu floats, the layout has %zu", cap, *n_floats);
}
