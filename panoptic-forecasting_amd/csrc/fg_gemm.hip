// fg forecaster, hot path: one implicit-GEMM core on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate = the reference's precision),
//   D[pixel][col] += A[pixel][k] * B[k][col],  rows = the 196 pixels of ONE instance's 14x14 plane (13 M-tiles of 16),
//   k = (channel, tap), 64 columns per workgroup.  Per round of KC channels the 16x16 halo planes are staged in LDS
//   (zero halo = padding 1) next to the matching 64-column slice of the packed weights.  The K sources are read in place:
//     vec  channels that are constant over the plane (traj_feat_out, fg_model.py:265-266): one float per instance,
//          written into the plane interior while staging - never expanded to 14x14 in memory;
//     x    a plane source (instance_feats[:, t], the lower layer's h, a mask-head activation);
//     h    h_prev; nullptr on the first step of a ConvLSTM (init_hidden: h = c = 0) -> that half of K is skipped.
//   The concatenation torch.cat([input, h]) (convlstm.py:47) is never built: the channel index picks the source.
//   Epilogues (template parameter of the same core):
//     EPI_LSTM    the columns of a tile are the i, f, o, g rows of 16 hidden channels (permuted at pack time), so a lane
//                 holds all four gates of one (pixel, channel): c' = s(f) c + s(i) tanh(g), h' = s(o) tanh(c') (:58-68);
//                 c stays fp32 in place; the gates are never stored
//     EPI_RELU    bias + ReLU (mask_fcn1..4, mask_rcnn_conv_upsample_head.py:60-65)
//     EPI_BIAS    bias (mask_encoder_out / mask_decoder_out, 1x1)
//     EPI_DECONV  ConvTranspose2d 2x2/s2 as a 1x1 GEMM 256 -> 1024 = (cout, dy, dx), stored as a pixel shuffle, + ReLU
//
// PF_FG_PAIR (pfhip.h) runs the 3x3 instantiations - the four ConvLSTM cells and mask_fcn1..4 - through pair_kernel instead: the same
// tiling and epilogues on v_mfma_f32_16x16x32_f16, every fp32 operand fed as two round-to-nearest fp16 terms (conv_mfma.h: split_terms2)
// with three products and fp32 accumulation.  Storage is unchanged (fp32 everywhere in memory); the split happens while staging.
#include "fg_net.h"
#include "pf_prof.h"

namespace pf {
namespace fg {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PS = 272;      // LDS plane stride (16x16 halo plane + 16: the four k-lanes of an A fragment hit distinct banks)

// Shared by the two cores as a function: the accumulator clear alone.  The M-tile pixel table, the resolution of the K sources and the
// epilogue stay written out in gemm_kernel: moved into helpers of any form tried (reference or value arguments, functor or lambda) they
// compile gemm_kernel to other instructions and other register counts (1x1: 98 / 97 -> 99 / 98 or 96 / 95 VGPRs; <9,relu> gains a spill
// with the table helper), pair_kernel's own pair_epilogue compiles the same either way
__device__ __forceinline__ void clear(f32x4 (&acc)[4][4]) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[m][g] = f32x4{0.f, 0.f, 0.f, 0.f};
}
// ------------------------------------------------------------------------------------------------------- fp32 core
template <int TAPS, int EPI>
__global__ __launch_bounds__(256, TAPS == 9 ? 4 : 1) void gemm_kernel(GemmArgs a) {
    constexpr int KC = TAPS == 9 ? 8 : 32;      // channels per LDS round
    constexpr int KR = KC * TAPS;               // k per round (72 / 32)
    __shared__ float xs[KC * PS];
    __shared__ __attribute__((aligned(16))) float ws[KR * 64];
    __shared__ int koff[KR];
    const int n = blockIdx.x, tile = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < KR) {
        const int cl = tid / TAPS, tap = tid % TAPS;
        koff[tid] = TAPS == 9 ? cl * PS + (tap / 3) * 16 + tap % 3 : cl * PS + 17;
    }
    int pb[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        int p = (wave + 4 * m) * 16 + (lane & 15);
        p = p < HW ? p : HW - 1;                // rows past the plane compute on pixel 195 and are never stored
        pb[m] = (p / 14) * 16 + p % 14;
    }
    f32x4 acc[4][4];
    clear(acc);

    const int cloop = a.nvec + a.nx + (a.h ? a.nh : 0);
    const float *wt = a.w + (size_t)tile * a.ctot * TAPS * 64;
    const float *vecn = a.vec ? a.vec + n * a.vec_stride : nullptr;
    const float *xn = a.x + n * a.x_stride;
    const float *hn = a.h ? a.h + n * a.h_stride : nullptr;
    for (int c0 = 0; c0 < cloop; c0 += KC) {
        __syncthreads();
        for (int i = tid; i < KC * 256; i += 256) {
            const int cl = i >> 8, r = i & 255, yy = r >> 4, xx = r & 15;
            const int c = c0 + cl;
            float v = 0.f;
            if (yy >= 1 && yy <= 14 && xx >= 1 && xx <= 14) {
                const int pix = (yy - 1) * 14 + xx - 1;
                if (c < a.nvec) v = vecn[c];
                else if (c < a.nvec + a.nx) v = xn[(c - a.nvec) * HW + pix];
                else v = hn[(c - a.nvec - a.nx) * HW + pix];
            }
            xs[cl * PS + r] = v;
        }
        const float4 *wsrc = reinterpret_cast<const float4 *>(wt + (size_t)c0 * TAPS * 64);
        for (int i = tid; i < KR * 16; i += 256) reinterpret_cast<float4 *>(ws)[i] = wsrc[i];
        __syncthreads();
        if (TAPS == 9) {
            // blocked sum: the 18 matrix steps of a round go into a partial of their own, added to acc once per round - one chain
            // over the whole K (up to 1188 steps on one accumulator) is 4x further from float64 than a blocked fp32 sum.
            // Two M-tiles at a time keep the partials at 32 registers (the weight fragments are read once per pair).  The
            // scheduling barrier, the un-unrolled step loop and the occupancy bound of 4 waves per SIMD (128 registers) keep the
            // compiler from holding both pairs' partials and several steps' fragments at once: 178 ... 227 registers and 2 waves
            // per SIMD without them, +38 % at N = 512; as written +5 % (N = 512) ... +8 % (N = 32) against the single chain
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                f32x4 part[2][4];
                auto step = [&](int ks, bool first) {
                    const int k = ks * 4 + (lane >> 4);
                    const int ko = koff[k];
                    float bf[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) bf[g] = ws[k * 64 + g * 16 + (lane & 15)];
#pragma unroll
                    for (int mm = 0; mm < 2; ++mm) {
                        if (wave + 4 * (2 * half + mm) < 13) {
                            const float af = xs[pb[2 * half + mm] + ko];
#pragma unroll
                            for (int g = 0; g < 4; ++g)
                                part[mm][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf[g], first ? f32x4{0.f, 0.f, 0.f, 0.f} : part[mm][g], 0, 0, 0);
                        }
                    }
                };
                step(0, true);
#pragma unroll 1
                for (int ks = 1; ks < KR / 4; ++ks) step(ks, false);
#pragma unroll
                for (int mm = 0; mm < 2; ++mm) {
                    if (wave + 4 * (2 * half + mm) >= 13) continue;
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[2 * half + mm][g] += part[mm][g];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll 2
            for (int ks = 0; ks < KR / 4; ++ks) {
                const int k = ks * 4 + (lane >> 4);
                const int ko = koff[k];
                float bf[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) bf[g] = ws[k * 64 + g * 16 + (lane & 15)];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    if (wave + 4 * m < 13) {
                        const float af = xs[pb[m] + ko];
#pragma unroll
                        for (int g = 0; g < 4; ++g) acc[m][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf[g], acc[m][g], 0, 0, 0);
                    }
                }
            }
        }
    }

    // epilogue: D[row = (lane>>4)*4 + r][col = lane & 15] of M-tile wave + 4m, column tile g
    const int col = lane & 15;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (wave + 4 * m >= 13) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = (wave + 4 * m) * 16 + (lane >> 4) * 4 + r;
            if (p >= HW) continue;
            if (EPI == EPI_LSTM) {
                const int j = tile * 16 + col;
                const float gi = sigm(acc[m][0][r] + a.bias[j]);
                const float gf = sigm(acc[m][1][r] + a.bias[C + j]);
                const float go = sigm(acc[m][2][r] + a.bias[2 * C + j]);
                const float gg = tanhf(acc[m][3][r] + a.bias[3 * C + j]);
                const size_t ci = ((size_t)n * C + j) * HW + p;
                const float cp = a.h ? a.c[ci] : 0.f;
                const float cn = gf * cp + gi * gg;
                a.c[ci] = cn;
                a.out[n * a.out_stride + (size_t)j * HW + p] = go * tanhf(cn);
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int q = tile * 64 + g * 16 + col;
                    if (EPI == EPI_DECONV) {
                        const int co = q >> 2, dy = (q >> 1) & 1, dx = q & 1;
                        const int y = p / 14, x = p % 14;
                        a.out[n * a.out_stride + (size_t)co * 784 + (2 * y + dy) * 28 + 2 * x + dx] =
                            fmaxf(acc[m][g][r] + a.bias[co], 0.f);
                    } else {
                        float v = acc[m][g][r] + a.bias[q];
                        if (EPI == EPI_RELU) v = fmaxf(v, 0.f);
                        a.out[n * a.out_stride + (size_t)q * HW + p] = v;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------- fp16-pair core (PF_FG_PAIR)
// The TAPS == 9 GEMM on v_mfma_f32_16x16x32_f16 - the only matrix shape these accumulators ever see.  Same workgroup tile as gemm_kernel
// (one instance's 13 M-tiles x 64 columns, M-tile wave + 4m), same three K sources read in place, same epilogues.  Per round of PKC = 16
// channels:
//   xs [term][16x16 halo pixel][16 ch] fp16   hi = fp16(x), mid = fp16(x - hi), split while staging; the halo is zeroed once
//   ws [term][tap][64 col][16 ch] fp16        a straight copy of the round's slice of the packed pair weights (w * 2^k)
// K order inside a round: tap-major, the 16 channels contiguous under each tap, so the 8 K-values of a lane are one 16-byte LDS read.  A
// matrix step covers two taps: lane group q = lane >> 4 holds channels 8 (q & 1) .. + 7 of tap 2 mf + (q >> 1).  Nine taps make 4.5
// steps: in the fifth, groups 2 and 3 multiply a zero A fragment (halo pixel 0) by tap 8's weights again.
// Consecutive pixels / columns are 32 B apart per term, so the 16 lanes of a ds_read_b128 group (MI355X: 8 rows of one channel octet and
// 8 of the other) cover the 16 slots of a bank row; only an M-tile's row ends (pixel index + 2) cost a 2-way conflict.
// Products hi*mid + mid*hi + hi*hi into a per-round partial, partials added to acc once per round (the blocked sum of gemm_kernel).
// Range guard (conv_mfma.h): the workgroups of column tile 0 - every tile stages the same planes - keep max |v| per K source and whether
// any value is not <= 65504; one atomic per source and workgroup into the launch's three slots of the status block.

// gemm_kernel's epilogue (EPI_LSTM, EPI_RELU; same D layout: the wide instruction puts D[row = (lane>>4)*4 + r][col = lane & 15] where the
// fp32 one does, so the i, f, o, g columns of a hidden channel still meet in one lane).  The raw sums are those of w * 2^k: sc = 2^-k
// enters in the bias addition (one fma: the product is exact)
template <int EPI>
__device__ __forceinline__ void pair_epilogue(const GemmArgs &a, const f32x4 (&acc)[4][4], int n, int tile, int wave, int lane, float sc) {
    auto pre = [&](float s, float b) { return fmaf(s, sc, b); };
    const int col = lane & 15;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (wave + 4 * m >= 13) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = (wave + 4 * m) * 16 + (lane >> 4) * 4 + r;
            if (p >= HW) continue;
            if (EPI == EPI_LSTM) {
                const int j = tile * 16 + col;
                const float gi = sigm(pre(acc[m][0][r], a.bias[j]));
                const float gf = sigm(pre(acc[m][1][r], a.bias[C + j]));
                const float go = sigm(pre(acc[m][2][r], a.bias[2 * C + j]));
                const float gg = tanhf(pre(acc[m][3][r], a.bias[3 * C + j]));
                const size_t ci = ((size_t)n * C + j) * HW + p;
                const float cp = a.h ? a.c[ci] : 0.f;
                const float cn = gf * cp + gi * gg;
                a.c[ci] = cn;
                a.out[n * a.out_stride + (size_t)j * HW + p] = go * tanhf(cn);
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int q = tile * 64 + g * 16 + col;
                    a.out[n * a.out_stride + (size_t)q * HW + p] = fmaxf(pre(acc[m][g][r], a.bias[q]), 0.f);      // EPI_RELU
                }
            }
        }
    }
}

template <int EPI>
__global__ __launch_bounds__(256, 2) void pair_kernel(PairArgs pa) {
    __shared__ __attribute__((aligned(16))) split_t xs[2 * PTERM_X];
    __shared__ __attribute__((aligned(16))) split_t ws[PROUND];
    __shared__ unsigned red[4];
    const GemmArgs &a = pa.g;
    const int n = blockIdx.x, tile = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool report = tile == 0 && pa.status != nullptr;
    if (tid < 4) red[tid] = 0u;
    for (int i = tid; i < 2 * PTERM_X / 8; i += 256) reinterpret_cast<split_x8 *>(xs)[i] = split_x8{0, 0, 0, 0, 0, 0, 0, 0};

    const int row = lane & 15, choct = (lane >> 4) & 1, tsel = lane >> 5;
    int aoff[5], boff[5];       // fp16 offsets of the lane's fragment in xs (behind the M-tile's pixel) and ws (behind the column tile)
#pragma unroll
    for (int mf = 0; mf < 5; ++mf) {
        const int tap = 2 * mf + tsel;
        aoff[mf] = ((tap / 3) * 16 + tap % 3) * PKC + choct * 8;
        boff[mf] = ((tap < 9 ? tap : 8) * 64 + row) * PKC + choct * 8;
    }
    int pb[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        int p = (wave + 4 * m) * 16 + row;
        p = p < HW ? p : HW - 1;                // rows past the plane compute on pixel 195 and are never stored
        pb[m] = ((p / 14) * 16 + p % 14) * PKC;
    }
    f32x4 acc[4][4];
    clear(acc);

    const int cloop = a.nvec + a.nx + (a.h ? a.nh : 0);
    const int rounds = (a.ctot + PKC - 1) / PKC;
    const split_t *wt = pa.wp + (size_t)tile * rounds * PROUND;
    const float *vecn = a.vec ? a.vec + n * a.vec_stride : nullptr;
    const float *xn = a.x + n * a.x_stride;
    const float *hn = a.h ? a.h + n * a.h_stride : nullptr;
    float smax[3] = {0.f, 0.f, 0.f};
    bool bad = false;
    for (int c0 = 0; c0 < cloop; c0 += PKC) {
        __syncthreads();
        // a task = one pixel's channel octet (the source boundaries are multiples of 8: one source per octet)
        for (int i = tid; i < 2 * HW; i += 256) {
            const int j = i >= HW, p = i - j * HW;
            const int c = c0 + 8 * j;
            float v[8];
            int src = -1;
            if (c >= cloop) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = 0.f;
            } else if (c < a.nvec) {
                src = 0;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = vecn[c + e];
            } else if (c < a.nvec + a.nx) {
                src = 1;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = xn[(c - a.nvec + e) * HW + p];
            } else {
                src = 2;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = hn[(c - a.nvec - a.nx + e) * HW + p];
            }
            if (report && src >= 0) {
                float m = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    m = fmaxf(m, fabsf(v[e]));
                    bad |= !(fabsf(v[e]) <= kSplitMaxAbs);
                }
                if (src == 0) smax[0] = fmaxf(smax[0], m);
                else if (src == 1) smax[1] = fmaxf(smax[1], m);
                else smax[2] = fmaxf(smax[2], m);
            }
            split_x2 h2[4], m2[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) split_terms2(v[2 * e], v[2 * e + 1], h2[e], m2[e]);
            const int at = ((p / 14 + 1) * 16 + p % 14 + 1) * PKC + 8 * j;
            *reinterpret_cast<split_x8 *>(xs + at) = split_x8{h2[0][0], h2[0][1], h2[1][0], h2[1][1], h2[2][0], h2[2][1], h2[3][0], h2[3][1]};
            *reinterpret_cast<split_x8 *>(xs + PTERM_X + at) = split_x8{m2[0][0], m2[0][1], m2[1][0], m2[1][1], m2[2][0], m2[2][1], m2[3][0], m2[3][1]};
        }
        const split_x8 *wsrc = reinterpret_cast<const split_x8 *>(wt + (size_t)(c0 / PKC) * PROUND);
        for (int i = tid; i < PROUND / 8; i += 256) reinterpret_cast<split_x8 *>(ws)[i] = wsrc[i];
        __syncthreads();
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            f32x4 part[2][4];
#pragma unroll
            for (int mm = 0; mm < 2; ++mm)
#pragma unroll
                for (int g = 0; g < 4; ++g) part[mm][g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int mf = 0; mf < 5; ++mf) {
                split_x8 bh[4], bm[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    bh[g] = *reinterpret_cast<const split_x8 *>(ws + boff[mf] + g * 16 * PKC);
                    bm[g] = *reinterpret_cast<const split_x8 *>(ws + PTERM_W + boff[mf] + g * 16 * PKC);
                }
#pragma unroll
                for (int mm = 0; mm < 2; ++mm) {
                    const int m = 2 * half + mm;
                    if (wave + 4 * m < 13) {
                        const int ao = (mf == 4 && tsel) ? choct * 8 : pb[m] + aoff[mf];      // tap 9 does not exist: zero halo pixel
                        const split_x8 ah = *reinterpret_cast<const split_x8 *>(xs + ao);
                        const split_x8 am = *reinterpret_cast<const split_x8 *>(xs + PTERM_X + ao);
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            part[mm][g] = PF_MFMA_SPLIT(ah, bm[g], part[mm][g]);
                            part[mm][g] = PF_MFMA_SPLIT(am, bh[g], part[mm][g]);
                            part[mm][g] = PF_MFMA_SPLIT(ah, bh[g], part[mm][g]);
                        }
                    }
                }
                // one step's fragments at a time: left alone the compiler hoists all five steps' reads (160 registers) and spills
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int mm = 0; mm < 2; ++mm) {
                if (wave + 4 * (2 * half + mm) >= 13) continue;
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[2 * half + mm][g] += part[mm][g];
            }
        }
    }
    if (report) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (smax[k] > 0.f) atomicMax(&red[k], __builtin_bit_cast(unsigned, smax[k]));
        if (bad) atomicOr(&red[3], 1u);
        __syncthreads();
        if (tid < 3 && red[tid] != 0u) atomicMax(pa.slots + tid, red[tid]);
        if (tid == 3 && red[3] != 0u) atomicOr(pa.status, 1u);      // PF_STATUS_RANGE
    }
    pair_epilogue<EPI>(a, acc, n, tile, wave, lane, *pa.scale);
}

// Status block of a PF_FG_PAIR workspace: word 0 = this forward's PF_STATUS_* bits, word 1 = OR over the forwards since the host cleared
// it, words 2, 3 = what pf_fg_status copies out, words FG_SLOT0 .. = the slots.  A slot that is non-zero and below kRangeLowMax is a K
// source that was tiny over a whole launch: PF_STATUS_RANGE_LOW.  The slots are judged by whoever comes next - the following forward's
// first launch (begin = 1: fold into word 1, zero word 0 and the slots) or pf_fg_status (begin = 0: fold, copy out, clear both words)
__global__ __launch_bounds__(FG_STATUS_WORDS) void status_kernel(unsigned *st, int begin) {
    __shared__ unsigned low;
    const int tid = threadIdx.x;
    if (tid == 0) low = 0u;
    __syncthreads();
    if (tid >= FG_SLOT0) {
        const unsigned v = st[tid];
        if (v != 0u && v < __builtin_bit_cast(unsigned, kRangeLowMax)) atomicOr(&low, 2u);      // PF_STATUS_RANGE_LOW
        st[tid] = 0u;
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned w0 = st[0] | low, w1 = st[1] | w0;
        if (!begin) st[2] = w0, st[3] = w1;
        st[0] = 0u;
        st[1] = begin ? w1 : 0u;
    }
}

// ------------------------------------------------------------------------------------------------------------- launchers
int launch_status(unsigned *st, int begin, hipStream_t s) {
    hipLaunchKernelGGL(status_kernel, dim3(1), dim3(FG_STATUS_WORDS), 0, s, st, begin);
    PF_LAUNCH_CHECK("status_kernel");
    return 0;
}

// flops: the fp32-equivalent work (one product per operand pair), for either core
static ProfScope gemm_scope(const GemmArgs &a, int taps, int N, int tiles, const char *label, hipStream_t s) {
    const double cols = tiles * 64.0, planes = a.nx + (a.h ? a.nh : 0);
    return ProfScope(s, label, 2.0 * N * HW * cols * (a.nvec + planes) * taps, 4.0 * N * (planes * HW + cols * HW));
}

int launch_gemm(const GemmArgs &a, int taps, int epi, int N, int tiles, const char *label, hipStream_t s) {
    ProfScope ps = gemm_scope(a, taps, N, tiles, label, s);
    const dim3 grid(N, tiles), block(256);
    if (taps == 9 && epi == EPI_LSTM) hipLaunchKernelGGL((gemm_kernel<9, EPI_LSTM>), grid, block, 0, s, a);
    else if (taps == 9 && epi == EPI_RELU) hipLaunchKernelGGL((gemm_kernel<9, EPI_RELU>), grid, block, 0, s, a);
    else if (taps == 1 && epi == EPI_BIAS) hipLaunchKernelGGL((gemm_kernel<1, EPI_BIAS>), grid, block, 0, s, a);
    else if (taps == 1 && epi == EPI_DECONV) hipLaunchKernelGGL((gemm_kernel<1, EPI_DECONV>), grid, block, 0, s, a);
    else return fail(PF_EINVAL, "pf_fg: %s: no gemm_kernel<%d,%d>", label, taps, epi);
    PF_LAUNCH_CHECK(label);
    return 0;
}

int launch_pair(const PairArgs &pa, int epi, int N, int tiles, const char *label, hipStream_t s) {
    ProfScope ps = gemm_scope(pa.g, 9, N, tiles, label, s);
    const dim3 grid(N, tiles), block(256);
    if (epi == EPI_LSTM) hipLaunchKernelGGL((pair_kernel<EPI_LSTM>), grid, block, 0, s, pa);
    else if (epi == EPI_RELU) hipLaunchKernelGGL((pair_kernel<EPI_RELU>), grid, block, 0, s, pa);
    else return fail(PF_EINVAL, "pf_fg: %s: no pair_kernel<%d>", label, epi);
    PF_LAUNCH_CHECK(label);
    return 0;
}

}  // namespace fg
}  // namespace pf
