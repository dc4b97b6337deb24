// What builds the network input of the bg model (HBM/L2-bound, VALU only):
//   stem_onehot_kernel, _v3, _v4 : bg_model.py:53-69 (one-hot, depth normalise, concat) fused with the stem conv hardnet.py base.0
//                        (3x3 s2, BN folded, ReLU).  The [B,36,H,W] tensor is never built: a one-hot channel contributes exactly one
//                        weight column per tap, so the conv is a gather-sum of 16-wide weight rows from LDS.  Optionally emulates the
//                        reference's on-disk hop (export_cityscapes_segmentation_results.py:34-38,119-124 and
//                        bg_dataset.py:224-230,166-170) on the fly.  net_select.cpp (choose_stem) says which of them a launch runs.
//   dense_input_kernel : the same tensor written out, for the configurations the fused stem does not cover
#include "net_kernels.h"
#include "conv_epilogue.h"
#include "pf_prof.h"

namespace pf {

// The on-disk hop of a depth value in registers: quantise to the u16 code of the export (:119-124), load it back (bg_dataset.py:225),
// mask and clamp (:227-228, :166-170) -> the depth, m = its mask.  (Not hop_decode.h: that one decodes a stored code and clamps the
// upper bound first; this chain re-quantises a float, lower bound first - their bits are pinned by different tests.)
__device__ __forceinline__ float hop_depth(float d, float min_depth, float max_depth, float &m) {
    const float q = rintf(fminf(fmaxf(d + 1.f, 0.f), 255.f) * 256.f);
    d = q / 256.f - 1.f;
    const bool mk = d > 0.f;
    d = mk ? fminf(fmaxf(d, min_depth), max_depth) : -1.f;
    m = mk ? 1.f : 0.f;
    return d;
}

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stem_onehot_kernel(StemArgs a) {
    // weights in LDS as [tap][ch][16]: row = one input channel's 16 output weights for that tap
    extern __shared__ __attribute__((aligned(16))) float wl[];
    __shared__ uint8_t lut[256];
    const int in_ch = a.T * (a.n_cls + 1);
    for (int e = threadIdx.x; e < 9 * in_ch * 16; e += 256) {
        const int co = e & 15, ch = (e >> 4) % in_ch, tap = (e >> 4) / in_ch;
        wl[e] = a.w[((size_t)co * in_ch + ch) * 9 + tap];
    }
    lut[threadIdx.x] = (a.hop & PF_HOP_TRAINID_LUT) ? a.lut[threadIdx.x] : (uint8_t)threadIdx.x;
    __syncthreads();

    const int ox = blockIdx.x * 64 + (threadIdx.x & 63);
    const int oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.z;
    if (ox >= a.Wout || oy >= a.Hout) return;
    const size_t N = (size_t)a.H * a.W;
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = a.bias[i];
    const float mean_ = a.depth_mean, std_ = a.depth_std;

    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * 2 - 1 + ky;
        if (iy < 0 || iy >= a.H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * 2 - 1 + kx;
            if (ix < 0 || ix >= a.W) continue;
            const int tap = ky * 3 + kx;
            const size_t pix = (size_t)iy * a.W + ix;
            for (int t = 0; t < a.T; ++t) {
                const size_t idx = ((size_t)b * a.T + t) * N + pix;
                // label -> one-hot column (labels >= n_cls contribute nothing, bg_model.py:54-57)
                // (an int64 label is compared in 64 bits: 2^32 + 3 is no class; the LUT, which the reference applies to u8 files
                //  only, reads its low byte)
                long long lab = a.seg_is_i64 ? reinterpret_cast<const long long *>(a.seg)[idx]
                                             : (long long)reinterpret_cast<const uint8_t *>(a.seg)[idx];
                if (a.hop & PF_HOP_TRAINID_LUT) lab = lut[lab & 255];
                if (lab >= 0 && lab < a.n_cls) {
                    const int cls = (int)lab;
                    const f32x4v *row = reinterpret_cast<const f32x4v *>(wl + (tap * in_ch + t * a.n_cls + cls) * 16);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4v r = row[q];
                        acc[q * 4 + 0] += r[0]; acc[q * 4 + 1] += r[1]; acc[q * 4 + 2] += r[2]; acc[q * 4 + 3] += r[3];
                    }
                }
                // depth channel: ((d - mean)/std) * mask   (bg_model.py:50-51,66-67)
                float d = a.depth[idx];
                float m;
                if (a.hop & PF_HOP_DEPTH_U16) {                                          // hop_depth() written out: through the
                    // helper hipcc lays the branches of this kernel out differently, and its code is to stay as it is
                    const float q = rintf(fminf(fmaxf(d + 1.f, 0.f), 255.f) * 256.f);  // export :119-124
                    d = q / 256.f - 1.f;                                                // load bg_dataset.py:225
                    const bool mk = d > 0.f;
                    d = mk ? fminf(fmaxf(d, a.min_depth), a.max_depth) : -1.f;           // :227-228,:166-170
                    m = mk ? 1.f : 0.f;
                } else {
                    m = a.mask[idx] ? 1.f : 0.f;
                }
                const float dn = ((d - mean_) / std_) * m;
                const f32x4v *row = reinterpret_cast<const f32x4v *>(wl + (tap * in_ch + a.T * a.n_cls + t) * 16);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4v r = row[q];
                    acc[q * 4 + 0] += r[0] * dn; acc[q * 4 + 1] += r[1] * dn;
                    acc[q * 4 + 2] += r[2] * dn; acc[q * 4 + 3] += r[3] * dn;
                }
            }
        }
    }
    const size_t op = (size_t)a.Hout * a.Wout;
    float *o = a.dst + (size_t)b * 16 * op + (size_t)oy * a.Wout + ox;
    float vmax = 0.f;   // the output is >= 0 after the ReLU: range guard of the operand split (conv_mfma.h)
    bool nan = false;   // a NaN input propagates like in the reference's fp32 conv, but max() would drop it: flag it
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        o[i * op] = fmaxf(acc[i], 0.f);
        vmax = fmaxf(vmax, acc[i]);
        nan = nan || acc[i] != acc[i];
    }
    range_commit(a.status, a.range_slot, nan ? __builtin_inff() : vmax);
}

// ------------------------------------------------------------------------------------------------
// Stem, T = 3 compile-time.  The generic kernel above walks its 9*T taps one dependent load -> LUT -> weight-row chain at a
// time (54 serial HBM round trips per wave; profiles/r01_e: 193 us at B=4 for 65 us of traffic), computes a 64-bit address
// for each of the 54 loads of a lane, branches per (tap, frame) around the one-hot row, and every workgroup gathers its 20 KB
// of weights from the OIHW array 4 bytes at a time.  Here
//   * the one-hot rows arrive pre-packed [tap][t][n_cls + 1][16] (plan creation; the last row of each group is zero) and are
//     copied to LDS with 16-B loads; a label outside 0..n_cls-1 (or a tap outside the image) selects the zero row: no branch;
//   * the depth-channel weights are uniform per (tap, t) and come through the scalar cache (a.wdep, [tap][t][16]);
//   * loads use one uniform base per tensor + a 32-bit lane offset (T*H*W >= 2^32 goes to the generic kernel, which indexes
//     with size_t);
//   * accumulation is on register pairs (v_pk_add_f32 for the one-hot rows, v_pk_fma_f32 with scalar weight pairs for depth).
// Same operations on the same values in the same order as the generic kernel: outputs are bit-identical.
typedef float f32x2v __attribute__((ext_vector_type(2)));
template <int T, bool SEG64, bool HOP_D, bool HOP_LUT>
__global__ __launch_bounds__(256) void stem_onehot_v3_kernel(StemArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wl[];   // [tap][t][n_cls + 1][kStemRow]
    __shared__ uint8_t lut[256];
    const int rows_per = a.n_cls + 1;
    {
        const f32x4v *src = reinterpret_cast<const f32x4v *>(a.woh);
        f32x4v *dst = reinterpret_cast<f32x4v *>(wl);
        // (kStemRow = 20 would pad the rows so that lanes picking different rows never share a bank group)
        for (int e = threadIdx.x; e < 9 * T * rows_per * 4; e += 256) dst[(e >> 2) * (kStemRow / 4) + (e & 3)] = src[e];
    }
    lut[threadIdx.x] = HOP_LUT ? a.lut[threadIdx.x] : (uint8_t)threadIdx.x;
    __syncthreads();

    const int ox = blockIdx.x * 64 + (threadIdx.x & 63);
    const int oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.z;
    if (ox >= a.Wout || oy >= a.Hout) return;
    const unsigned N = (unsigned)a.H * (unsigned)a.W;
    constexpr bool hop_d = HOP_D;
    // uniform bases of this sample; lane offsets in elements (T*N < 2^32 is checked at launch)
    const uint8_t *seg8 = reinterpret_cast<const uint8_t *>(a.seg) + (size_t)b * T * N;
    const long long *seg64 = reinterpret_cast<const long long *>(a.seg) + (size_t)b * T * N;
    const float *depth = a.depth + (size_t)b * T * N;
    const uint8_t *mask = a.mask ? a.mask + (size_t)b * T * N : nullptr;
    // One (tap) per iteration of a ROLLED loop, the loads of the next three taps in flight (registers rotate).  Fully
    // unrolled, hipcc issues all 216 LDS row reads of the straight-line code first and spills them (512 registers +
    // scratch; scheduling fences do not stop it); the rolled loop holds 24 reads.
    struct Tap { int lab[T]; float dep[T]; uint8_t msk[T]; bool ok; };
    auto issue = [&](int tap, Tap &p) {
        const int ky = tap / 3, kx = tap - ky * 3;
        const int iy = oy * 2 - 1 + ky, ix = ox * 2 - 1 + kx;
        p.ok = tap < 9 && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        const unsigned pix = p.ok ? (unsigned)iy * (unsigned)a.W + (unsigned)ix : 0u;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const unsigned idx = (unsigned)t * N + pix;
            if (SEG64) {
                // compared in 64 bits before narrowing (2^32 + 3 is no class): n_cls stands for every label outside
                // 0..n_cls-1; the LUT, which the reference applies to u8 files only, reads the low byte
                const long long v = seg64[idx];
                p.lab[t] = HOP_LUT ? (int)(v & 255) : ((unsigned long long)v < (unsigned long long)a.n_cls ? (int)v : a.n_cls);
            } else {
                p.lab[t] = (int)seg8[idx];
            }
            p.dep[t] = depth[idx];
            p.msk[t] = hop_d ? (uint8_t)0 : mask[idx];
        }
    };
    f32x2v acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = f32x2v{a.bias[2 * i], a.bias[2 * i + 1]};
    const float mean_ = a.depth_mean, std_ = a.depth_std;
    Tap c0, c1, c2, c3;
    issue(0, c0);
    issue(1, c1);
    issue(2, c2);
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        issue(tap + 3 < 9 ? tap + 3 : 8, c3);
        const float *wrow = wl + tap * T * rows_per * kStemRow;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            int cls = c0.lab[t];
            if (HOP_LUT) cls = lut[cls & 255];
            // labels >= n_cls contribute nothing (bg_model.py:54-57): they, and taps outside the image, read the zero row
            const int r = (c0.ok && (unsigned)cls < (unsigned)a.n_cls) ? cls : a.n_cls;
            const f32x4v *row = reinterpret_cast<const f32x4v *>(wrow + (t * rows_per + r) * kStemRow);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4v w4 = row[q];
                acc[2 * q] += f32x2v{w4[0], w4[1]};
                acc[2 * q + 1] += f32x2v{w4[2], w4[3]};
            }
            float d = c0.dep[t], m;
            if (hop_d) {
                d = hop_depth(d, a.min_depth, a.max_depth, m);
            } else {
                m = c0.msk[t] ? 1.f : 0.f;
            }
            const float dn = c0.ok ? ((d - mean_) / std_) * m : 0.f;                 // (bg_model.py:50-51,66-67)
            const float *wd = a.wdep + (tap * T + t) * 16;                           // uniform: scalar loads, SGPR-pair operands
            const f32x2v dn2 = f32x2v{dn, dn};
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = __builtin_elementwise_fma(f32x2v{wd[2 * i], wd[2 * i + 1]}, dn2, acc[i]);
        }
        // the LDS row reads stay inside their iteration (hipcc otherwise rotates the loop and carries 12 rows = 48 registers
        // across the back edge: one wave per SIMD less); their ~100 cycles are hidden by the other waves
        __builtin_amdgcn_sched_barrier(0);
        c0 = c1;
        c1 = c2;
        c2 = c3;
    }
    const size_t op = (size_t)a.Hout * a.Wout;
    float *o = a.dst + (size_t)b * 16 * op + (size_t)oy * a.Wout + ox;
    float vmax = 0.f;   // range guard of the operand split (conv_mfma.h)
    bool nan = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        o[(2 * i) * op] = fmaxf(acc[i].x, 0.f);
        o[(2 * i + 1) * op] = fmaxf(acc[i].y, 0.f);
        vmax = fmaxf(vmax, fmaxf(acc[i].x, acc[i].y));
        nan = nan || acc[i].x != acc[i].x || acc[i].y != acc[i].y;
    }
    range_commit(a.status, a.range_slot, nan ? __builtin_inff() : vmax);
}

// ------------------------------------------------------------------------------------------------
// Stem, 2 x 2 outputs per lane (u8 labels; HOP_D: in-register depth hop - the fused forecast model - else depth + mask planes).
// stem_onehot_v3_kernel is 82 % vector-ALU-busy (PMC) and most of its instructions are not arithmetic on the accumulators:
// a lane evaluates the label -> row and depth -> hop -> normalise chain for all 9 x T taps of ITS output pixel, although a
// stride-2 3x3 window shares 5 of its 9 columns/rows with the neighbouring outputs - every input pixel goes through the
// chain 2.25 times - and it issues 2 loads per tap and frame (54 per output pixel).  Here a lane owns the outputs
// (oy0..oy0+1) x (ox0..ox0+1): their windows cover 5 x 5 input pixels, so
//   * the chain runs once per input pixel and frame: 75 instead of 108 evaluations per 4 outputs;
//   * the five pixels of a window row are ONE aligned 4-byte (labels) / 16-byte (depth) load plus the left neighbour:
//     4 load instructions per row and frame, 15 per output pixel instead of 54;
//   * an input pixel is accumulated into the 1-4 (output, tap) pairs it belongs to; which output ROWS an input row feeds
//     (row 2 feeds both) is wave-uniform: scalar branches in a rolled loop over the 5 input rows.
// For every output the operations and their order are those of v3 (ky, kx, t ascending; one-hot row, then depth): the
// results are bit-identical.  FAST_DIV: (d - mean) / std as q = x*r, q += fma(-q, std, x) * r with r = 1/std - correctly
// rounded for every value the hop chain can produce, which choose_stem() proves by trying all 65 281 of them on the host
// (net_select.cpp: stem_fast_div_exact) before it selects this variant.
// (134 registers = 3 waves per SIMD; capped at 128 for 4 waves it measures the same 342 us with 5 spills)
template <int T, bool HOP_D, bool HOP_LUT, bool FAST_DIV>
__global__ __launch_bounds__(256) void stem_onehot_v4_kernel(StemArgs a, float inv_std) {
    extern __shared__ __attribute__((aligned(16))) float wl[];   // [tap][t][n_cls + 1][16]
    __shared__ uint8_t lut[256];
    const int rows_per = a.n_cls + 1;
    {
        const f32x4v *src = reinterpret_cast<const f32x4v *>(a.woh);
        f32x4v *dst = reinterpret_cast<f32x4v *>(wl);
        for (int e = threadIdx.x; e < 9 * T * rows_per * 4; e += 256) dst[e] = src[e];
    }
    lut[threadIdx.x] = HOP_LUT ? a.lut[threadIdx.x] : (uint8_t)threadIdx.x;
    __syncthreads();

    const int ox0 = blockIdx.x * 128 + 2 * (threadIdx.x & 63);
    const int oy0 = blockIdx.y * 8 + 2 * (threadIdx.x >> 6);
    const int b = blockIdx.z;
    if (ox0 >= a.Wout || oy0 >= a.Hout) return;          // Wout, Hout even and W = 2 Wout, H = 2 Hout (checked at launch)
    const unsigned N = (unsigned)a.H * (unsigned)a.W;
    const uint8_t *seg8 = reinterpret_cast<const uint8_t *>(a.seg) + (size_t)b * T * N;
    const float *depth = a.depth + (size_t)b * T * N;
    const uint8_t *mask = HOP_D ? nullptr : a.mask + (size_t)b * T * N;
    const int ix0 = 2 * ox0;                               // multiple of 4: window columns ix0 - 1 .. ix0 + 3
    const bool left_ok = ix0 > 0;
    struct Row { unsigned lab4[T], labl[T], msk4[T], mskl[T]; f32x4v dep4[T]; float depl[T]; bool ok; };
    auto issue = [&](int r, Row &p) {
        const int iy = 2 * oy0 - 1 + r;                    // <= H - 1 for r <= 4
        p.ok = iy >= 0;
        const unsigned row = (unsigned)(p.ok ? iy : 0) * (unsigned)a.W + (unsigned)ix0;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const unsigned idx = (unsigned)t * N + row;
            p.lab4[t] = *reinterpret_cast<const unsigned *>(seg8 + idx);
            p.dep4[t] = *reinterpret_cast<const f32x4v *>(depth + idx);
            const unsigned il = left_ok ? idx - 1u : idx;
            p.labl[t] = seg8[il];
            p.depl[t] = depth[il];
            p.msk4[t] = HOP_D ? 0u : *reinterpret_cast<const unsigned *>(mask + idx);
            p.mskl[t] = HOP_D ? 0u : (unsigned)mask[il];
        }
    };
    f32x2v acc[2][2][8];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[o >> 1][o & 1][i] = f32x2v{a.bias[2 * i], a.bias[2 * i + 1]};
    const float mean_ = a.depth_mean, std_ = a.depth_std;
    // one (output, tap) pair: the one-hot row of the label, then the depth channel - as in v3
    auto accum = [&](f32x2v (&ac)[8], const float *wrow, const float *wd, float dn) {
        const f32x4v *row = reinterpret_cast<const f32x4v *>(wrow);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4v w4 = row[q];
            ac[2 * q] += f32x2v{w4[0], w4[1]};
            ac[2 * q + 1] += f32x2v{w4[2], w4[3]};
        }
        const f32x2v dn2 = f32x2v{dn, dn};
#pragma unroll
        for (int i = 0; i < 8; ++i) ac[i] = __builtin_elementwise_fma(f32x2v{wd[2 * i], wd[2 * i + 1]}, dn2, ac[i]);
    };
    Row cur, nxt;
    issue(0, cur);
#pragma unroll 1
    for (int r = 0; r < 5; ++r) {
        issue(r < 4 ? r + 1 : 4, nxt);
        const bool f0 = r <= 2, f1 = r >= 2;               // input row r = tap row r of output row 0, r - 2 of output row 1
        const int tap0 = r * 3, tap1 = (r - 2) * 3;
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const bool okc = cur.ok && (c > 0 || left_ok);
#pragma unroll
            for (int t = 0; t < T; ++t) {
                int cls = c == 0 ? (int)cur.labl[t] : (int)((cur.lab4[t] >> (8 * (c == 0 ? 0 : c - 1))) & 255u);
                float d = c == 0 ? cur.depl[t] : cur.dep4[t][c == 0 ? 0 : c - 1];
                if (HOP_LUT) cls = lut[cls & 255];
                // labels >= n_cls contribute nothing (bg_model.py:54-57): they, and taps outside the image, read the zero row
                const int rowi = (okc && (unsigned)cls < (unsigned)a.n_cls) ? cls : a.n_cls;
                float m;
                if (HOP_D) {
                    d = hop_depth(d, a.min_depth, a.max_depth, m);
                } else {
                    const unsigned mb = c == 0 ? cur.mskl[t] : (cur.msk4[t] >> (8 * (c == 0 ? 0 : c - 1))) & 255u;
                    m = mb ? 1.f : 0.f;
                }
                float qn;
                if (FAST_DIV) {
                    const float x = d - mean_;
                    const float q0 = x * inv_std;
                    qn = __builtin_fmaf(__builtin_fmaf(-q0, std_, x), inv_std, q0);
                } else {
                    qn = (d - mean_) / std_;
                }
                const float dn = okc ? qn * m : 0.f;                                 // (bg_model.py:50-51,66-67)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int kx = c - 2 * dx;
                    if (kx < 0 || kx > 2) continue;
                    if (f0) accum(acc[0][dx], wl + (((tap0 + kx) * T + t) * rows_per + rowi) * 16, a.wdep + ((tap0 + kx) * T + t) * 16, dn);
                    if (f1) accum(acc[1][dx], wl + (((tap1 + kx) * T + t) * rows_per + rowi) * 16, a.wdep + ((tap1 + kx) * T + t) * 16, dn);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        cur = nxt;
    }
    const size_t op = (size_t)a.Hout * a.Wout;
    float vmax = 0.f;   // range guard of the operand split (conv_mfma.h): base.1 reads this tensor through conv_split
    if (!HOP_D) {
        // a NaN depth (the hop chain cannot produce one: its clamp absorbs it) propagates through the reference's fp32 conv; here
        // the ReLU's max would turn it into 0: the sum of all accumulators is NaN iff one of them is (or two infinities cancel)
        f32x2v sum = f32x2v{0.f, 0.f};
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int i = 0; i < 8; ++i) sum += acc[o >> 1][o & 1][i];
        const float s1 = sum.x + sum.y;
        if (s1 != s1) vmax = __builtin_inff();
    }
    if (a.dst_fmt) {
        // packed pairs for the fused front kernel (conv_front.hip): per term and channel group one 16-B unit [2 px][4 ch]
        char *base = reinterpret_cast<char *>(a.dst) + (size_t)b * 2 * 4 * op * 8;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const size_t pix = (size_t)(oy0 + dy) * a.Wout + ox0;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4v v0, v1;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    v0[2 * h] = fmaxf(acc[dy][0][2 * g + h].x, 0.f); v0[2 * h + 1] = fmaxf(acc[dy][0][2 * g + h].y, 0.f);
                    v1[2 * h] = fmaxf(acc[dy][1][2 * g + h].x, 0.f); v1[2 * h + 1] = fmaxf(acc[dy][1][2 * g + h].y, 0.f);
                }
                vmax = range_acc(range_acc(vmax, v0[0], v0[1], v0[2], v0[3]), v1[0], v1[1], v1[2], v1[3]);
                split_x4 h0, m0, h1, m1;
                split_terms4(v0, h0, m0);
                split_terms4(v1, h1, m1);
                char *p = base + ((size_t)g * op + pix) * 8;
                *reinterpret_cast<split_x8 *>(p) = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
                *reinterpret_cast<split_x8 *>(p + (size_t)4 * op * 8) = __builtin_shufflevector(m0, m1, 0, 1, 2, 3, 4, 5, 6, 7);
            }
        }
        range_commit(a.status, a.range_slot, vmax);
        return;
    }
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        float *o = a.dst + (size_t)b * 16 * op + (size_t)(oy0 + dy) * a.Wout + ox0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            *reinterpret_cast<f32x2v *>(o + (2 * i) * op) = f32x2v{fmaxf(acc[dy][0][i].x, 0.f), fmaxf(acc[dy][1][i].x, 0.f)};
            *reinterpret_cast<f32x2v *>(o + (2 * i + 1) * op) = f32x2v{fmaxf(acc[dy][0][i].y, 0.f), fmaxf(acc[dy][1][i].y, 0.f)};
            vmax = range_acc(vmax, acc[dy][0][i].x, acc[dy][1][i].x, acc[dy][0][i].y, acc[dy][1][i].y);
        }
    }
    range_commit(a.status, a.range_slot, vmax);
}

// ------------------------------------------------------------------------------------------------
int launch_stem(const StemArgs &a, hipStream_t s) {
    StemChoice c;
    if (int rc = choose_stem(a, &c)) return rc;
    const double ipx = (double)a.B * a.T * a.H * a.W, opx = (double)a.B * a.Hout * a.Wout;
    const double flops = 2.0 * opx * 16 * a.T * (a.n_cls + 1) * 9;
    const double bytes = ipx * ((a.seg_is_i64 ? 8 : 1) + 4 + (c.hop_d ? 0 : 1)) + opx * 16 * 4;
    {
        ProfScope ps(s, c.label, flops, bytes);
        switch (c.family * 8 + c.variant) {   // the instantiation of the chosen row of the instance lists (net_kernels.h)
#define X(V, HD, HL, FD) \
    case STEM_V4 * 8 + V: hipLaunchKernelGGL((stem_onehot_v4_kernel<3, HD, HL, FD>), c.grid, dim3(kNetBlock), c.lds, s, a, 1.0f / a.depth_std); break;
            PF_STEM_V4_INSTANCES(X)
#undef X
#define X(V, S64, HD, HL) \
    case STEM_V3 * 8 + V: hipLaunchKernelGGL((stem_onehot_v3_kernel<3, S64, HD, HL>), c.grid, dim3(kNetBlock), c.lds, s, a); break;
            PF_STEM_V3_INSTANCES(X)
#undef X
            default: hipLaunchKernelGGL(stem_onehot_kernel, c.grid, dim3(kNetBlock), c.lds, s, a);
        }
    }
    PF_LAUNCH_CHECK("stem_onehot_kernel");
    return PF_OK;
}

// ------------------------------------------------------------------------------------------------ dense network input
// bg_model.py:61-69 for the configurations the fused stem does not cover (convert2onehot = False: frames that are images or
// already one-hot; or no depth channels): x[b, t * C + c] = frame channel c (labels: (label == c), labels >= n_cls -> zero
// vector, :53-59), then - with depth - x[b, T * C + t] = (depth - mean) / std * mask (IEEE division, like ATen).  Round 6: was ATen glue.
template <int KIND>   // 0: u8 labels, 1: i64 labels, 2: f32 frames [B][T][C][H][W]
__global__ __launch_bounds__(256) void dense_input_kernel(const void *frames, int C, const float *depth, const uint8_t *mask, float mean,
                                                          float stdv, int T, long long HW, float *x) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int bt = blockIdx.y, b = bt / T, t = bt - b * T;
    if (i >= HW) return;
    const int Cx = T * C + (depth ? T : 0);
    float *xb = x + (long long)b * Cx * HW + i;
    if (KIND == 2) {
        const float *f = reinterpret_cast<const float *>(frames) + (long long)bt * C * HW + i;
        for (int c = 0; c < C; ++c) xb[(long long)(t * C + c) * HW] = f[(long long)c * HW];
    } else {
        const long long in = (long long)bt * HW + i;
        const long long lab = KIND == 1 ? reinterpret_cast<const long long *>(frames)[in] : (long long)reinterpret_cast<const uint8_t *>(frames)[in];
        for (int c = 0; c < C; ++c) xb[(long long)(t * C + c) * HW] = (lab == c) ? 1.f : 0.f;
    }
    if (depth) {
        const long long in = (long long)bt * HW + i;
        xb[(long long)(T * C + t) * HW] = ((depth[in] - mean) / stdv) * (mask[in] ? 1.f : 0.f);
    }
}
}  // namespace pf

extern "C" int pf_bg_dense_input(const void *frames, int kind, int channels, const float *depth, const uint8_t *depth_mask, float depth_mean,
                                 float depth_std, int B, int T, int H, int W, float *x, void *stream) {
    if (!frames || !x || B <= 0 || T <= 0 || H <= 0 || W <= 0 || channels <= 0 || kind < 0 || kind > 2 || (depth && !depth_mask))
        return pf::fail(PF_EINVAL, "pf_bg_dense_input: bad argument (kind %d, channels %d, B %d T %d %dx%d)", kind, channels, B, T, H, W);
    const long long HW = (long long)H * W;
    const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)(B * T));
    hipStream_t s = (hipStream_t)stream;
    if (kind == 0) hipLaunchKernelGGL(pf::dense_input_kernel<0>, grid, dim3(256), 0, s, frames, channels, depth, depth_mask, depth_mean, depth_std, T, HW, x);
    else if (kind == 1) hipLaunchKernelGGL(pf::dense_input_kernel<1>, grid, dim3(256), 0, s, frames, channels, depth, depth_mask, depth_mean, depth_std, T, HW, x);
    else hipLaunchKernelGGL(pf::dense_input_kernel<2>, grid, dim3(256), 0, s, frames, channels, depth, depth_mask, depth_mean, depth_std, T, HW, x);
    PF_LAUNCH_CHECK("dense_input_kernel");
    return PF_OK;
}
