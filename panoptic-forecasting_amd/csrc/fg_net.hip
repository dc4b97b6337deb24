// fg forecaster network (FGModel.forward, models/fg/fg_model.py:216-339, shipped config) on gfx950.
//
// Hot path: one implicit-GEMM core on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate = the reference's precision),
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
// The trajectory path (GRU, normalisation, output MLPs) and the instance feature model are small VALU kernels.
// Every launch is a kernel node (no memset, no memcpy): a pf_fg_forward call can be captured into a graph.
//
// PF_FG_PAIR (pfhip.h) runs the 3x3 instantiations - the four ConvLSTM cells and mask_fcn1..4 - through pair_kernel instead: the same
// tiling and epilogues on v_mfma_f32_16x16x32_f16, every fp32 operand fed as two round-to-nearest fp16 terms (conv_mfma.h: split_terms2)
// with three products and fp32 accumulation.  Storage is unchanged (fp32 everywhere in memory); the split happens while staging.
#include "conv_mfma.h"
#include "pf_common.h"
#include "pf_prof.h"

namespace pf {
namespace fg {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int HW = 196;      // 14 x 14
constexpr int C = 256;       // mask feature / hidden channels
constexpr int HID = 128;     // GRU hidden size
constexpr int TR = 10;       // trajectory values: 8 box + 2 depth
constexpr int OD = 5;        // odometry values
constexpr int TF = 16;       // traj_feat_channels
constexpr int IFH = 64;      // instance_feat_hidden
constexpr int ICC = 8;       // instance_feat_channels
constexpr int PS = 272;      // LDS plane stride (16x16 halo plane + 16: the four k-lanes of an A fragment hit distinct banks)

// the 52 state_dict tensors, in the reference's state_dict order (= the order of the raw buffer handed to pf_fg_pack)
enum {
    ODOM_MEAN, ODOM_STD, DEPTH_MEAN, DEPTH_STD, TRAJ_MEAN, TRAJ_STD,
    TE_WIH, TE_WHH, TE_BIH, TE_BHH, TD_WIH, TD_WHH, TD_BIH, TD_BHH,
    TEO_W0, TEO_B0, TEO_W2, TEO_B2, TDO_W0, TDO_B0, TDO_W2, TDO_B2, TFO_W, TFO_B,
    IC_W, IC_B, IF_W, IF_B,
    ME0_W, ME0_B, ME1_W, ME1_B, MD0_W, MD0_B, MD1_W, MD1_B,
    MEO_W, MEO_B, MDO_W, MDO_B,
    F1_W, F1_B, F2_W, F2_B, F3_W, F3_B, F4_W, F4_B, DC_W, DC_B, PR_W, PR_B, NTENSOR
};
static const long long kSize[NTENSOR] = {
    OD, OD, 2, 2, 8, 8,
    3 * HID * 80, 3 * HID * HID, 3 * HID, 3 * HID, 3 * HID * 79, 3 * HID * HID, 3 * HID, 3 * HID,
    HID * HID, HID, TR * HID, TR, HID * HID, HID, TR * HID, TR, TF * HID, TF,
    ICC * C, ICC, IFH * ICC * HW, IFH,
    4LL * C * 528 * 9, 4 * C, 4LL * C * 512 * 9, 4 * C, 4LL * C * 528 * 9, 4 * C, 4LL * C * 512 * 9, 4 * C,
    C * C, C, C * C, C,
    C * C * 9, C, C * C * 9, C, C * C * 9, C, C * C * 9, C, C * C * 4, C, 8 * C, 8};

// GEMMs whose weights are packed [tile][K][64] behind the raw copy
enum { G_ME0, G_ME1, G_MD0, G_MD1, G_MEO, G_MDO, G_F1, G_F2, G_F3, G_F4, G_DC, NGEMM };
enum { MAP_LSTM = 0, MAP_PLAIN = 1, MAP_KMAJOR = 2 };
struct GemmDesc {
    int src, ctot, taps, tiles, map;
};
static const GemmDesc kGemm[NGEMM] = {
    {ME0_W, 528, 9, 16, MAP_LSTM}, {ME1_W, 512, 9, 16, MAP_LSTM}, {MD0_W, 528, 9, 16, MAP_LSTM}, {MD1_W, 512, 9, 16, MAP_LSTM},
    {MEO_W, 256, 1, 4, MAP_PLAIN}, {MDO_W, 256, 1, 4, MAP_PLAIN},
    {F1_W, 256, 9, 4, MAP_PLAIN}, {F2_W, 256, 9, 4, MAP_PLAIN}, {F3_W, 256, 9, 4, MAP_PLAIN}, {F4_W, 256, 9, 4, MAP_PLAIN},
    {DC_W, 256, 1, 16, MAP_KMAJOR}};

struct Layout {
    size_t raw[NTENSOR], raw_total, gemm[NGEMM], total;
};
static Layout layout() {
    Layout L;
    size_t o = 0;
    for (int i = 0; i < NTENSOR; ++i) {
        L.raw[i] = o;
        o += (size_t)kSize[i];
    }
    L.raw_total = o;
    o = align_up(o, 64);
    for (int g = 0; g < NGEMM; ++g) {
        L.gemm[g] = o;
        o += (size_t)kGemm[g].tiles * 64 * kGemm[g].ctot * kGemm[g].taps;
    }
    L.total = o;
    return L;
}

// ------------------------------------------------------------------------------------------------------------- packing
// packed[tile][k][q] = W[row(tile, q)][k]  (MAP_LSTM: row = gate*256 + tile*16 + q%16, gate = q/16; MAP_PLAIN: row = tile*64+q);
// MAP_KMAJOR (ConvTranspose2d [cin][cout*4]): packed[tile][k][q] = W[k][tile*64 + q]
__global__ __launch_bounds__(256) void pack_kernel(const float *__restrict__ w, float *__restrict__ out, int K, int tiles, int map) {
    const long long total = (long long)tiles * K * 64;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int q = (int)(i & 63);
        const long long tk = i >> 6;
        const int k = (int)(tk % K), tile = (int)(tk / K);
        float v;
        if (map == MAP_KMAJOR) {
            v = w[(long long)k * tiles * 64 + tile * 64 + q];
        } else {
            const int row = map == MAP_LSTM ? (q >> 4) * C + tile * 16 + (q & 15) : tile * 64 + q;
            v = w[(long long)row * K + k];
        }
        out[i] = v;
    }
}

// PF_FG_PAIR: behind the flags = 0 layout (kept whole: the 1x1 GEMMs and the deconvolution read it) a pair section,
//   [0 .. 7]  max |w| of the eight 3x3 GEMMs (bit patterns)   [8 .. 15]  their 2^-k   (64 floats)
//   then per 3x3 GEMM [tile][round of 16 channels][term hi, mid][tap][64 columns][16 channels] fp16 of w * 2^k, zero past ctot
// k = the rule of split_weight_scale (conv_mfma.h): max |w * 2^k| in [2^14, 2^15), k = 0 for an all-zero (or non-finite) tensor; the
// weights live on the device, so the maximum is a reduction kernel and k is derived from it by every packing thread.  |k| <= 120 keeps
// 2^k and 2^-k normal numbers (a tensor whose maximum is below 2^-106 is then scaled less than the rule says; both scalings stay exact)
constexpr int PKC = 16;                            // channels per round of pair_kernel
constexpr int PTERM_X = 256 * PKC;                 // fp16 per term of its activation planes in LDS
constexpr int PTERM_W = 9 * 64 * PKC;              // fp16 per term of a round's weights
constexpr int PROUND = 2 * PTERM_W;                // fp16 per (tile, round) of the packed pair weights
constexpr int NPAIR = 8;
static const int kPairGemm[NPAIR] = {G_ME0, G_ME1, G_MD0, G_MD1, G_F1, G_F2, G_F3, G_F4};
struct PairLayout {
    size_t head, gemm[NPAIR], total;    // floats from the start of the packed buffer
};
static size_t pair_rounds(int ctot) { return (size_t)(ctot + PKC - 1) / PKC; }
static PairLayout pair_layout(const Layout &L) {
    PairLayout P;
    size_t o = align_up(L.total, 64);
    P.head = o;
    o += 64;
    for (int i = 0; i < NPAIR; ++i) {
        const GemmDesc &d = kGemm[kPairGemm[i]];
        P.gemm[i] = o;
        o += (size_t)d.tiles * pair_rounds(d.ctot) * PROUND / 2;
    }
    P.total = o;
    return P;
}

__global__ __launch_bounds__(256) void absmax_kernel(const float *__restrict__ w, long long n, unsigned *__restrict__ out) {
    __shared__ unsigned m;
    if (threadIdx.x == 0) m = 0u;
    __syncthreads();
    float v = 0.f;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) v = fmaxf(v, fabsf(w[i]));
    atomicMax(&m, __builtin_bit_cast(unsigned, v));
    __syncthreads();
    if (threadIdx.x == 0 && m != 0u) atomicMax(out, m);
}

__device__ __forceinline__ int pair_exponent(unsigned maxbits) {
    const float m = __builtin_bit_cast(float, maxbits);
    if (!(m > 0.f) || !(m <= 3.4028234e38f)) return 0;
    const int k = 14 - ilogbf(m);
    return k < -120 ? -120 : (k > 120 ? 120 : k);
}

__global__ __launch_bounds__(256) void pack_pair_kernel(const float *__restrict__ w, _Float16 *__restrict__ out, int ctot, int tiles, int map,
                                                        const unsigned *__restrict__ maxbits, float *__restrict__ scale) {
    const int k = pair_exponent(*maxbits);
    if (blockIdx.x == 0 && threadIdx.x == 0) *scale = ldexpf(1.f, -k);
    const int rounds = (ctot + PKC - 1) / PKC, K = ctot * 9;
    const long long total = (long long)tiles * rounds * PTERM_W;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % PKC), q = (int)(i / PKC % 64);
        const long long t = i / (64 * PKC);
        const int tap = (int)(t % 9);
        const long long tr = t / 9;
        const int round = (int)(tr % rounds), tile = (int)(tr / rounds);
        const int c = round * PKC + ch;
        float v = 0.f;
        if (c < ctot) {
            const int row = map == MAP_LSTM ? (q >> 4) * C + tile * 16 + (q & 15) : tile * 64 + q;
            v = ldexpf(w[(long long)row * K + c * 9 + tap], k);
        }
        const _Float16 hi = (_Float16)v;
        const _Float16 mid = (_Float16)(v - (float)hi);
        const long long at = tr * PROUND + (tap * 64 + q) * PKC + ch;
        out[at] = hi;
        out[at + PTERM_W] = mid;
    }
}

// ------------------------------------------------------------------------------------------------------- GEMM core
enum { EPI_LSTM = 0, EPI_RELU = 1, EPI_BIAS = 2, EPI_DECONV = 3 };

struct GemmArgs {
    const float *vec;           // [n*vec_stride + c], c < nvec
    long long vec_stride;
    int nvec;
    const float *x;             // [n*x_stride + c*196 + p], c < nx
    long long x_stride;
    int nx;
    const float *h;             // [n*h_stride + c*196 + p], c < nh; nullptr: zero state (K half skipped, c_prev = 0)
    long long h_stride;
    int nh;
    int ctot;                   // channels of the packed K (nvec + nx + nh)
    const float *w;             // packed [tiles][ctot*TAPS][64]
    const float *bias;
    float *out;                 // EPI_LSTM: h' [n*out_stride + j*196 + p]; EPI_DECONV: [n*out_stride + co*784 + 28y' + x']
    long long out_stride;
    float *c;                   // EPI_LSTM: cell state [n][256][196], updated in place
};

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }

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
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[m][g] = f32x4{0.f, 0.f, 0.f, 0.f};

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
constexpr int FG_STATUS_WORDS = 256;               // status block at the head of a PF_FG_PAIR workspace
constexpr int FG_SLOT0 = 8;                        // its words 8 ..: max |v| bit patterns, three (vec, x, h) per pair launch

struct PairArgs {
    GemmArgs g;                 // g.w unused
    const split_t *wp;          // [tile][round][term][tap][64][16] fp16 terms of w * 2^k, zero past ctot
    const float *scale;         // 2^-k (device: k is found on the device at pack time)
    unsigned *status;           // word 0 of the status block
    unsigned *slots;            // this launch's three slots
};

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
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[m][g] = f32x4{0.f, 0.f, 0.f, 0.f};

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

// ------------------------------------------------------------------------------------------------ small VALU kernels
// _compute_traj_inst_feats (fg_model.py:206-214): relu(instance_compressor(x)) flattened channel-major -> instance_feat_model
// -> * mask.  One workgroup per (instance, step); x plane of step t at x + n*x_stride + t*t_stride.
__global__ __launch_bounds__(256) void inst_feat_kernel(const float *__restrict__ x, long long x_stride, long long t_stride,
                                                        const float *__restrict__ mask, int T, const float *__restrict__ wc,
                                                        const float *__restrict__ bc, const float *__restrict__ wf,
                                                        const float *__restrict__ bfv, float *__restrict__ out) {
    __shared__ float comp[ICC * HW];
    __shared__ float wcs[ICC * C];
    __shared__ float part[256];
    const int n = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const float *xp = x + n * x_stride + t * t_stride;
    for (int i = tid; i < ICC * C; i += 256) wcs[i] = wc[i];
    __syncthreads();
    if (tid < HW) {
        float s[ICC];
#pragma unroll
        for (int o = 0; o < ICC; ++o) s[o] = bc[o];
        for (int ci = 0; ci < C; ++ci) {
            const float v = xp[ci * HW + tid];
#pragma unroll
            for (int o = 0; o < ICC; ++o) s[o] = fmaf(wcs[o * C + ci], v, s[o]);
        }
#pragma unroll
        for (int o = 0; o < ICC; ++o) comp[o * HW + tid] = fmaxf(s[o], 0.f);
    }
    __syncthreads();
    const int o = tid >> 2, q = tid & 3;
    float s = 0.f;
    for (int i = q; i < ICC * HW; i += 4) s = fmaf(wf[o * ICC * HW + i], comp[i], s);
    part[tid] = s;
    __syncthreads();
    if (q == 0) {
        const float m = mask ? mask[n * T + t] : 1.f;
        out[((size_t)n * T + t) * IFH + o] = (part[tid] + part[tid + 1] + part[tid + 2] + part[tid + 3] + bfv[o]) * m;
    }
}

// One GRU step (nn.GRU, gate order r, z, n; b_hn inside r*(...)) for a workgroup of >= H threads: x[nin], h[H] in LDS;
// thread j < H returns h'_j.  Shared by the encoder and the decoder (and by any later GRU of the same form).
__device__ float gru_step(const float *x, int nin, const float *h, int H, const float *__restrict__ wih,
                          const float *__restrict__ whh, const float *__restrict__ bih, const float *__restrict__ bhh, int j) {
    float ir = bih[j], iz = bih[H + j], in_ = bih[2 * H + j];
    for (int k = 0; k < nin; ++k) {
        const float v = x[k];
        ir = fmaf(wih[(size_t)j * nin + k], v, ir);
        iz = fmaf(wih[(size_t)(H + j) * nin + k], v, iz);
        in_ = fmaf(wih[(size_t)(2 * H + j) * nin + k], v, in_);
    }
    float hr = bhh[j], hz = bhh[H + j], hn = bhh[2 * H + j];
    for (int k = 0; k < H; ++k) {
        const float v = h[k];
        hr = fmaf(whh[(size_t)j * H + k], v, hr);
        hz = fmaf(whh[(size_t)(H + j) * H + k], v, hz);
        hn = fmaf(whh[(size_t)(2 * H + j) * H + k], v, hn);
    }
    const float r = sigm(ir + hr), z = sigm(iz + hz);
    const float nn = tanhf(in_ + r * hn);
    return (1.f - z) * nn + z * h[j];
}

__device__ float dot_row(const float *__restrict__ w, const float *v, int n, float acc) {
    for (int k = 0; k < n; ++k) acc = fmaf(w[k], v[k], acc);
    return acc;
}

struct TrajArgs {
    const float *trajs, *traj_mask, *vel_mask, *depths, *depth_mask, *odom;
    int T_in, T_out, odom_T;
    const float *instf;         // [N][T_in][64] (encoder) / [N][64] (decoder)
    float *gru_h;               // [N][128]
    float *tfeat;               // [N][T_in][16] (encoder) / [N][16] (decoder)
    float *traj_norm, *traj_unnorm;     // [N][1+T_out][10]
    int step;                   // decoder step
    // resolved raw offsets
    const float *odom_mean, *odom_std, *depth_mean, *depth_std, *traj_mean, *traj_std;
    const float *wih, *whh, *bih, *bhh, *w0, *b0, *w2, *b2, *wtf, *btf;
};

__device__ void traj_head(const TrajArgs &a, const float *h, float *hid, const float *prev, int slot, int n, int tid) {
    // traj_*_out (Linear, ReLU, Linear) of h, + prev (the residual current_traj + out, :309) when prev != nullptr
    hid[tid] = fmaxf(dot_row(a.w0 + tid * HID, h, HID, a.b0[tid]), 0.f);
    __syncthreads();
    if (tid < TR) {
        float v = dot_row(a.w2 + tid * HID, hid, HID, a.b2[tid]);
        if (prev) v += prev[tid];
        const size_t o = ((size_t)n * (1 + a.T_out) + slot) * TR + tid;
        a.traj_norm[o] = v;
        const float mean = tid < 8 ? a.traj_mean[tid] : a.depth_mean[tid - 8];
        const float sd = tid < 8 ? a.traj_std[tid] : a.depth_std[tid - 8];
        a.traj_unnorm[o] = v * sd + mean;
    }
}

// encoder (fg_model.py:236-275, 281): normalisation :167-204 + expand_traj_mask (model_utils.py:11-27), T_in GRU steps from
// h = 0, traj_feat_out of every step, traj_encoder_out of the last one
__global__ __launch_bounds__(HID) void traj_encoder_kernel(TrajArgs a) {
    __shared__ float xin[80], h[HID], hid[HID];
    const int n = blockIdx.x, tid = threadIdx.x;
    h[tid] = 0.f;
    for (int t = 0; t < a.T_in; ++t) {
        const int nt = n * a.T_in + t;
        if (tid < TR) {
            const float m = a.traj_mask[nt];
            const float dm = a.depth_mask[nt];
            float mk, v, mean, sd;
            if (tid < 4) mk = m;
            else if (tid < 8) mk = a.vel_mask[nt];
            else if (tid == 8) mk = dm;
            else mk = t > 0 ? dm * a.depth_mask[nt - 1] : 0.f;
            if (tid < 8) {
                v = a.trajs[nt * 8 + tid];
                mean = a.traj_mean[tid];
                sd = a.traj_std[tid];
            } else {
                v = a.depths[nt * 2 + tid - 8];
                mean = a.depth_mean[tid - 8];
                sd = a.depth_std[tid - 8];
            }
            xin[tid] = (v - mean) / sd * mk;
        } else if (tid < TR + IFH) {
            xin[tid] = a.instf[(size_t)nt * IFH + tid - TR];
        } else if (tid == TR + IFH) {
            xin[tid] = a.traj_mask[nt];
        } else if (tid < TR + IFH + 1 + OD) {
            const int k = tid - TR - IFH - 1;
            xin[tid] = (a.odom[((size_t)n * a.odom_T + t) * OD + k] - a.odom_mean[k]) / a.odom_std[k];
        }
        __syncthreads();
        const float hn = gru_step(xin, 80, h, HID, a.wih, a.whh, a.bih, a.bhh, tid);
        __syncthreads();
        h[tid] = hn;
        __syncthreads();
        if (tid < TF) a.tfeat[(size_t)nt * TF + tid] = dot_row(a.wtf + tid * HID, h, HID, a.btf[tid]);
    }
    a.gru_h[(size_t)n * HID + tid] = h[tid];
    traj_head(a, h, hid, nullptr, 0, n, tid);
}

// one decoder step (fg_model.py:289-309): input [current_traj, traj_inst_feats, out_odom[t]], GRU, current_traj + out,
// traj_feat_out of the new state (:295-296)
__global__ __launch_bounds__(HID) void traj_decoder_kernel(TrajArgs a) {
    __shared__ float xin[79], h[HID], hid[HID], cur[TR];
    const int n = blockIdx.x, tid = threadIdx.x, t = a.step;
    h[tid] = a.gru_h[(size_t)n * HID + tid];
    if (tid < TR) {
        cur[tid] = a.traj_norm[((size_t)n * (1 + a.T_out) + t) * TR + tid];
        xin[tid] = cur[tid];
    } else if (tid < TR + IFH) {
        xin[tid] = a.instf[(size_t)n * IFH + tid - TR];
    } else if (tid < TR + IFH + OD) {
        const int k = tid - TR - IFH;
        xin[tid] = (a.odom[((size_t)n * a.odom_T + a.T_in + t) * OD + k] - a.odom_mean[k]) / a.odom_std[k];
    }
    __syncthreads();
    const float hn = gru_step(xin, 79, h, HID, a.wih, a.whh, a.bih, a.bhh, tid);
    __syncthreads();
    h[tid] = hn;
    a.gru_h[(size_t)n * HID + tid] = hn;
    __syncthreads();
    if (tid < TF) a.tfeat[(size_t)n * TF + tid] = dot_row(a.wtf + tid * HID, h, HID, a.btf[tid]);
    traj_head(a, h, hid, cur, t + 1, n, tid);
}

// output_feats = mask_feats[:, -T_out:][range(N), output_inds] (:334); indices are clamped into [0, T_out)
__global__ __launch_bounds__(256) void gather_kernel(const float *__restrict__ mf, const int64_t *__restrict__ sel, int T_out,
                                                     float *__restrict__ out) {
    const int n = blockIdx.x;
    long long s = sel[n];
    s = s < 0 ? 0 : (s >= T_out ? T_out - 1 : s);
    const float4 *src = reinterpret_cast<const float4 *>(mf + ((size_t)n * (1 + T_out) + 1 + s) * C * HW);
    float4 *dst = reinterpret_cast<float4 *>(out + (size_t)n * C * HW);
    for (int i = threadIdx.x; i < C * HW / 4; i += 256) dst[i] = src[i];
}

// predictor row of each instance's class only (:335-336): masks[n] = W[cls] . y[n] + b[cls]; classes clamped into [0, 8)
__global__ __launch_bounds__(256) void predictor_kernel(const float *__restrict__ y, const int64_t *__restrict__ cls,
                                                        const float *__restrict__ w, const float *__restrict__ b,
                                                        float *__restrict__ out) {
    __shared__ float wr[C];
    const int n = blockIdx.x, tid = threadIdx.x;
    long long k = cls[n];
    k = k < 0 ? 0 : (k > 7 ? 7 : k);
    wr[tid] = w[k * C + tid];
    __syncthreads();
    const float *yn = y + (size_t)n * C * 784;
    for (int p = tid; p < 784; p += 256) {
        float s = b[k];
        for (int c = 0; c < C; ++c) s = fmaf(wr[c], yn[c * 784 + p], s);
        out[(size_t)n * 784 + p] = s;
    }
}

// ----------------------------------------------------------------------------------------------------------- host
struct Ws {
    size_t instf, instd, gruh, tfe, tfd, h0, c0, h1, c1, ya, yb, yd, total;
    int r0;
};
static Ws ws_layout(int N, int T_in) {
    Ws w;
    const size_t P = (size_t)N * C * HW;
    size_t o = 0;
    auto take = [&](size_t floats) {
        size_t at = o;
        o = align_up(o + floats, 64);
        return at;
    };
    w.r0 = T_in > 2 ? T_in : 2;
    w.instf = take((size_t)N * T_in * IFH);
    w.instd = take((size_t)N * IFH);
    w.gruh = take((size_t)N * HID);
    w.tfe = take((size_t)N * T_in * TF);
    w.tfd = take((size_t)N * TF);
    w.h0 = take(P * w.r0);
    w.c0 = take(P);
    w.h1 = take(2 * P);
    w.c1 = take(P);
    w.ya = take(P);
    w.yb = take(P);
    w.yd = take((size_t)N * C * 784);
    w.total = o * sizeof(float);
    return w;
}

static int check_dims(int N, int T_in, int T_out, int flags, int known = PF_FG_PAIR) {
    if (flags & ~known) return fail(PF_EUNSUPPORTED, "pf_fg: unsupported flags 0x%x (only the shipped fg configuration is built; PF_FG_PAIR is the one switch)", flags);
    if (N < 0 || N > (1 << 20) || T_in < 1 || T_in > 16 || T_out < 1 || T_out > 16)
        return fail(PF_EINVAL, "pf_fg: bad dims N=%d T_in=%d T_out=%d", N, T_in, T_out);
    return 0;
}

template <int TAPS, int EPI>
static int launch_gemm(const GemmArgs &a, int N, int tiles, const char *label, hipStream_t s) {
    const double cols = tiles * 64.0;
    const double k = (double)(a.nvec + a.nx + (a.h ? a.nh : 0)) * TAPS;
    ProfScope ps(s, label, 2.0 * N * HW * cols * k, 4.0 * N * ((a.nx + (a.h ? a.nh : 0)) * HW + cols * HW));
    hipLaunchKernelGGL((gemm_kernel<TAPS, EPI>), dim3(N, tiles), dim3(256), 0, s, a);
    PF_LAUNCH_CHECK(label);
    return 0;
}

// the 3x3 GEMMs of a forward: gemm_kernel<9, EPI>, or pair_kernel<EPI> when the forward runs under PF_FG_PAIR (pc != nullptr)
struct PairCtx {
    const float *packed;
    PairLayout P;
    unsigned *st;       // status block
    int launch;         // pair launches so far: picks the slots
};
static int pair_index(int gemm) {
    for (int i = 0; i < NPAIR; ++i)
        if (kPairGemm[i] == gemm) return i;
    return -1;
}
template <int EPI>
static int launch_conv3(const GemmArgs &a, int N, int tiles, int gemm, const char *label, const char *pair_label, PairCtx *pc, hipStream_t s) {
    if (!pc) return launch_gemm<9, EPI>(a, N, tiles, label, s);
    const int i = pair_index(gemm);
    if (i < 0 || a.nvec % 8 || a.nx % 8 || a.nh % 8 || FG_SLOT0 + 3 * (pc->launch + 1) > FG_STATUS_WORDS)
        return fail(PF_EINVAL, "pf_fg: %s has no pair form", label);
    PairArgs pa = {};
    pa.g = a;
    pa.wp = reinterpret_cast<const split_t *>(pc->packed + pc->P.gemm[i]);
    pa.scale = pc->packed + pc->P.head + 8 + i;
    pa.status = pc->st;
    pa.slots = pc->st + FG_SLOT0 + 3 * pc->launch++;
    const double cols = tiles * 64.0;
    const int cin = a.nvec + a.nx + (a.h ? a.nh : 0);
    // flops: the fp32-equivalent work (one product per operand pair), as gemm_kernel counts it
    ProfScope ps(s, pair_label, 2.0 * N * HW * cols * cin * 9, 4.0 * N * ((a.nx + (a.h ? a.nh : 0)) * HW + cols * HW));
    hipLaunchKernelGGL((pair_kernel<EPI>), dim3(N, tiles), dim3(256), 0, s, pa);
    PF_LAUNCH_CHECK(pair_label);
    return 0;
}

}  // namespace fg
}  // namespace pf

using namespace pf;
using namespace pf::fg;

extern "C" int pf_fg_weights_size(int flags, size_t *raw_floats, size_t *packed_floats) {
    if (!raw_floats || !packed_floats) return fail(PF_EINVAL, "pf_fg_weights_size: null output");
    if (int rc = check_dims(0, 1, 1, flags)) return rc;
    const Layout L = layout();
    *raw_floats = L.raw_total;
    *packed_floats = (flags & PF_FG_PAIR) ? pair_layout(L).total : L.total;
    return 0;
}

extern "C" int pf_fg_pack(const float *raw, float *packed, int flags, void *stream) {
    if (int rc = check_dims(0, 1, 1, flags)) return rc;
    if (!raw || !packed) return fail(PF_EINVAL, "pf_fg_pack: null buffer");
    hipStream_t s = (hipStream_t)stream;
    const Layout L = layout();
    if (int rc = launch_copy(packed, raw, L.raw_total * sizeof(float), s)) return rc;
    for (int g = 0; g < NGEMM; ++g) {
        const GemmDesc &d = kGemm[g];
        hipLaunchKernelGGL(pack_kernel, dim3(1024), dim3(256), 0, s, raw + L.raw[d.src], packed + L.gemm[g], d.ctot * d.taps,
                           d.tiles, d.map);
        PF_LAUNCH_CHECK("pf_fg_pack");
    }
    if (flags & PF_FG_PAIR) {
        const PairLayout P = pair_layout(L);
        unsigned *head = reinterpret_cast<unsigned *>(packed + P.head);
        if (int rc = launch_zero_fill(head, 64 * sizeof(float), s)) return rc;
        for (int i = 0; i < NPAIR; ++i) {
            const GemmDesc &d = kGemm[kPairGemm[i]];
            const long long n = (long long)d.tiles * 64 * d.ctot * d.taps;
            hipLaunchKernelGGL(absmax_kernel, dim3(256), dim3(256), 0, s, raw + L.raw[d.src], n, head + i);
            PF_LAUNCH_CHECK("pf_fg_pack");
            hipLaunchKernelGGL(pack_pair_kernel, dim3(1024), dim3(256), 0, s, raw + L.raw[d.src], reinterpret_cast<_Float16 *>(packed + P.gemm[i]),
                               d.ctot, d.tiles, d.map, head + i, packed + P.head + 8 + i);
            PF_LAUNCH_CHECK("pf_fg_pack");
        }
    }
    return 0;
}

extern "C" int pf_fg_workspace(int N, int T_in, int T_out, int flags, size_t *bytes) {
    if (!bytes) return fail(PF_EINVAL, "pf_fg_workspace: null output");
    // flags = 0 only, as ever: the workspace of a PF_FG_PAIR forward has a size call of its own
    if (int rc = check_dims(N, T_in, T_out, flags, 0)) return rc;
    *bytes = ws_layout(N, T_in).total;
    return 0;
}

extern "C" int pf_fg_pair_workspace(int N, int T_in, int T_out, size_t *bytes) {
    if (!bytes) return fail(PF_EINVAL, "pf_fg_pair_workspace: null output");
    if (int rc = check_dims(N, T_in, T_out, PF_FG_PAIR)) return rc;
    *bytes = ws_layout(N, T_in).total + FG_STATUS_WORDS * sizeof(unsigned);
    return 0;
}

extern "C" int pf_fg_forward(const float *packed, int flags, int N, int T_in, int T_out, int odom_T, const float *trajs,
                             const float *traj_mask, const float *vel_mask, const float *feats, const int64_t *output_inds,
                             const float *odom, const float *depths, const float *depth_mask, const int64_t *classes,
                             float *traj_norm, float *traj_unnorm, float *mask_feats, float *output_feats, float *masks,
                             void *ws, size_t ws_bytes, void *stream) {
    if (int rc = check_dims(N, T_in, T_out, flags)) return rc;
    if (odom_T < T_in + T_out) return fail(PF_EINVAL, "pf_fg_forward: odometry has %d steps, needs T_in + T_out = %d", odom_T, T_in + T_out);
    const Ws W = ws_layout(N, T_in);
    if (N == 0) return 0;      // nothing to forecast: no launch
    if (!packed || !trajs || !traj_mask || !vel_mask || !feats || !output_inds || !odom || !depths || !depth_mask || !classes ||
        !traj_norm || !traj_unnorm || !mask_feats || !output_feats || !masks || !ws)
        return fail(PF_EINVAL, "pf_fg_forward: null buffer");
    const size_t status_bytes = (flags & PF_FG_PAIR) ? FG_STATUS_WORDS * sizeof(unsigned) : 0;
    if (ws_bytes < W.total + status_bytes)
        return fail(PF_EWORKSPACE, "pf_fg_forward: workspace %zu < %zu bytes", ws_bytes, W.total + status_bytes);
    hipStream_t s = (hipStream_t)stream;
    const Layout L = layout();
    const float *R = packed;
    float *wsf = (float *)((char *)ws + status_bytes);
    PairCtx pair_ctx = {packed, pair_layout(L), (unsigned *)ws, 0};
    PairCtx *pc = (flags & PF_FG_PAIR) ? &pair_ctx : nullptr;
    if (pc) {       // the forward's first launch: last forward's slots judged, word 0 and the slots zeroed (a kernel, never a memset node)
        hipLaunchKernelGGL(status_kernel, dim3(1), dim3(FG_STATUS_WORDS), 0, s, pc->st, 1);
        PF_LAUNCH_CHECK("status_kernel");
    }
    const size_t P = (size_t)N * C * HW;
    const long long mf_stride = (long long)(1 + T_out) * C * HW;

    TrajArgs ta = {};
    ta.trajs = trajs, ta.traj_mask = traj_mask, ta.vel_mask = vel_mask, ta.depths = depths, ta.depth_mask = depth_mask;
    ta.odom = odom, ta.T_in = T_in, ta.T_out = T_out, ta.odom_T = odom_T;
    ta.gru_h = wsf + W.gruh;
    ta.traj_norm = traj_norm, ta.traj_unnorm = traj_unnorm;
    ta.odom_mean = R + L.raw[ODOM_MEAN], ta.odom_std = R + L.raw[ODOM_STD];
    ta.depth_mean = R + L.raw[DEPTH_MEAN], ta.depth_std = R + L.raw[DEPTH_STD];
    ta.traj_mean = R + L.raw[TRAJ_MEAN], ta.traj_std = R + L.raw[TRAJ_STD];
    ta.wtf = R + L.raw[TFO_W], ta.btf = R + L.raw[TFO_B];

    // ---- encoder: instance features of the T_in input steps (times the step mask), trajectory GRU
    {
        ProfScope ps(s, "pf::fg::inst_feat_kernel", 2.0 * N * T_in * (ICC * C * HW + IFH * ICC * HW), 4.0 * N * T_in * C * HW);
        hipLaunchKernelGGL(inst_feat_kernel, dim3(N, T_in), dim3(256), 0, s, feats, (long long)T_in * C * HW, (long long)C * HW,
                           traj_mask, T_in, R + L.raw[IC_W], R + L.raw[IC_B], R + L.raw[IF_W], R + L.raw[IF_B], wsf + W.instf);
        PF_LAUNCH_CHECK("inst_feat_kernel");
    }
    {
        TrajArgs e = ta;
        e.instf = wsf + W.instf, e.tfeat = wsf + W.tfe;
        e.wih = R + L.raw[TE_WIH], e.whh = R + L.raw[TE_WHH], e.bih = R + L.raw[TE_BIH], e.bhh = R + L.raw[TE_BHH];
        e.w0 = R + L.raw[TEO_W0], e.b0 = R + L.raw[TEO_B0], e.w2 = R + L.raw[TEO_W2], e.b2 = R + L.raw[TEO_B2];
        ProfScope ps(s, "pf::fg::traj_encoder_kernel", 2.0 * N * T_in * 3 * HID * (80 + HID), 0);
        hipLaunchKernelGGL(traj_encoder_kernel, dim3(N), dim3(HID), 0, s, e);
        PF_LAUNCH_CHECK("traj_encoder_kernel");
    }
    // ---- ConvLSTM encoder, layer-major like convlstm.py:150-166: layer 0 over all steps, then layer 1
    float *h0 = wsf + W.h0, *c0 = wsf + W.c0, *h1 = wsf + W.h1, *c1 = wsf + W.c1;
    for (int t = 0; t < T_in; ++t) {
        GemmArgs g = {};
        g.vec = wsf + W.tfe + (size_t)t * TF, g.vec_stride = (long long)T_in * TF, g.nvec = TF;
        g.x = feats + (size_t)t * C * HW, g.x_stride = (long long)T_in * C * HW, g.nx = C;
        g.h = t ? h0 + (t - 1) * P : nullptr, g.h_stride = (long long)C * HW, g.nh = C;
        g.ctot = TF + 2 * C, g.w = R + L.gemm[G_ME0], g.bias = R + L.raw[ME0_B];
        g.out = h0 + t * P, g.out_stride = (long long)C * HW, g.c = c0;
        if (int rc = launch_conv3<EPI_LSTM>(g, N, 16, G_ME0, "pf::fg::gemm_kernel<9,lstm> enc0", "pf::fg::pair_kernel<lstm> enc0", pc, s)) return rc;
    }
    int h1cur = -1;
    for (int t = 0; t < T_in; ++t) {
        GemmArgs g = {};
        g.x = h0 + t * P, g.x_stride = (long long)C * HW, g.nx = C;
        g.h = t ? h1 + h1cur * P : nullptr, g.h_stride = (long long)C * HW, g.nh = C;
        g.ctot = 2 * C, g.w = R + L.gemm[G_ME1], g.bias = R + L.raw[ME1_B];
        const int nxt = (h1cur + 1) & 1;
        g.out = h1 + nxt * P, g.out_stride = (long long)C * HW, g.c = c1;
        if (int rc = launch_conv3<EPI_LSTM>(g, N, 16, G_ME1, "pf::fg::gemm_kernel<9,lstm> enc1", "pf::fg::pair_kernel<lstm> enc1", pc, s)) return rc;
        h1cur = nxt;
    }
    int h0cur = T_in - 1;
    auto out_conv = [&](int which, int slot) {
        GemmArgs g = {};
        g.x = h1 + h1cur * P, g.x_stride = (long long)C * HW, g.nx = C;
        g.ctot = C, g.w = R + L.gemm[which == 0 ? G_MEO : G_MDO], g.bias = R + L.raw[which == 0 ? MEO_B : MDO_B];
        g.out = mask_feats + (size_t)slot * C * HW, g.out_stride = mf_stride;
        return launch_gemm<1, EPI_BIAS>(g, N, 4, "pf::fg::gemm_kernel<1,bias> out", s);
    };
    if (int rc = out_conv(0, 0)) return rc;                                          // current_mask_feats (:282-284)
    // ---- decoder (:289-318)
    for (int t = 0; t < T_out; ++t) {
        const float *cmf = mask_feats + (size_t)t * C * HW;                        // current_mask_feats, stride mf_stride
        {
            ProfScope ps(s, "pf::fg::inst_feat_kernel", 2.0 * N * (ICC * C * HW + IFH * ICC * HW), 4.0 * N * C * HW);
            hipLaunchKernelGGL(inst_feat_kernel, dim3(N, 1), dim3(256), 0, s, cmf, mf_stride, 0LL, (const float *)nullptr, 1,
                               R + L.raw[IC_W], R + L.raw[IC_B], R + L.raw[IF_W], R + L.raw[IF_B], wsf + W.instd);
            PF_LAUNCH_CHECK("inst_feat_kernel");
        }
        {
            TrajArgs d = ta;
            d.instf = wsf + W.instd, d.tfeat = wsf + W.tfd, d.step = t;
            d.wih = R + L.raw[TD_WIH], d.whh = R + L.raw[TD_WHH], d.bih = R + L.raw[TD_BIH], d.bhh = R + L.raw[TD_BHH];
            d.w0 = R + L.raw[TDO_W0], d.b0 = R + L.raw[TDO_B0], d.w2 = R + L.raw[TDO_W2], d.b2 = R + L.raw[TDO_B2];
            ProfScope ps(s, "pf::fg::traj_decoder_kernel", 2.0 * N * 3 * HID * (79 + HID), 0);
            hipLaunchKernelGGL(traj_decoder_kernel, dim3(N), dim3(HID), 0, s, d);
            PF_LAUNCH_CHECK("traj_decoder_kernel");
        }
        {
            GemmArgs g = {};
            g.vec = wsf + W.tfd, g.vec_stride = TF, g.nvec = TF;
            g.x = cmf, g.x_stride = mf_stride, g.nx = C;
            g.h = h0 + h0cur * P, g.h_stride = (long long)C * HW, g.nh = C;
            g.ctot = TF + 2 * C, g.w = R + L.gemm[G_MD0], g.bias = R + L.raw[MD0_B];
            const int nxt = (h0cur + 1) % W.r0;
            g.out = h0 + nxt * P, g.out_stride = (long long)C * HW, g.c = c0;
            if (int rc = launch_conv3<EPI_LSTM>(g, N, 16, G_MD0, "pf::fg::gemm_kernel<9,lstm> dec0", "pf::fg::pair_kernel<lstm> dec0", pc, s)) return rc;
            h0cur = nxt;
        }
        {
            GemmArgs g = {};
            g.x = h0 + h0cur * P, g.x_stride = (long long)C * HW, g.nx = C;
            g.h = h1 + h1cur * P, g.h_stride = (long long)C * HW, g.nh = C;
            g.ctot = 2 * C, g.w = R + L.gemm[G_MD1], g.bias = R + L.raw[MD1_B];
            const int nxt = (h1cur + 1) & 1;
            g.out = h1 + nxt * P, g.out_stride = (long long)C * HW, g.c = c1;
            if (int rc = launch_conv3<EPI_LSTM>(g, N, 16, G_MD1, "pf::fg::gemm_kernel<9,lstm> dec1", "pf::fg::pair_kernel<lstm> dec1", pc, s)) return rc;
            h1cur = nxt;
        }
        if (int rc = out_conv(1, t + 1)) return rc;
    }
    // ---- mask head on the selected step (:334-336)
    hipLaunchKernelGGL(gather_kernel, dim3(N), dim3(256), 0, s, mask_feats, output_inds, T_out, output_feats);
    PF_LAUNCH_CHECK("gather_kernel");
    float *ya = wsf + W.ya, *yb = wsf + W.yb;
    const float *src = output_feats;
    float *dsts[4] = {ya, yb, ya, yb};
    const int fw[4] = {G_F1, G_F2, G_F3, G_F4}, fb[4] = {F1_B, F2_B, F3_B, F4_B};
    for (int i = 0; i < 4; ++i) {
        GemmArgs g = {};
        g.x = src, g.x_stride = (long long)C * HW, g.nx = C;
        g.ctot = C, g.w = R + L.gemm[fw[i]], g.bias = R + L.raw[fb[i]];
        g.out = dsts[i], g.out_stride = (long long)C * HW;
        if (int rc = launch_conv3<EPI_RELU>(g, N, 4, fw[i], "pf::fg::gemm_kernel<9,relu> mask_fcn", "pf::fg::pair_kernel<relu> mask_fcn", pc, s)) return rc;
        src = dsts[i];
    }
    {
        GemmArgs g = {};
        g.x = src, g.x_stride = (long long)C * HW, g.nx = C;
        g.ctot = C, g.w = R + L.gemm[G_DC], g.bias = R + L.raw[DC_B];
        g.out = wsf + W.yd, g.out_stride = (long long)C * 784;
        if (int rc = launch_gemm<1, EPI_DECONV>(g, N, 16, "pf::fg::gemm_kernel<1,deconv>", s)) return rc;
    }
    {
        ProfScope ps(s, "pf::fg::predictor_kernel", 2.0 * N * 784 * C, 4.0 * N * 784 * C);
        hipLaunchKernelGGL(predictor_kernel, dim3(N), dim3(256), 0, s, wsf + W.yd, classes, R + L.raw[PR_W], R + L.raw[PR_B], masks);
        PF_LAUNCH_CHECK("predictor_kernel");
    }
    return 0;
}

extern "C" int pf_fg_status(void *ws, unsigned *out2, void *stream) {
    if (!ws || !out2) return fail(PF_EINVAL, "pf_fg_status: null argument");
    hipStream_t s = (hipStream_t)stream;
    unsigned *st = (unsigned *)ws;
    hipLaunchKernelGGL(status_kernel, dim3(1), dim3(FG_STATUS_WORDS), 0, s, st, 0);
    PF_LAUNCH_CHECK("status_kernel");
    if (hipMemcpyAsync(out2, st + 2, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(PF_EHIP, "pf_fg_status: reading the status words failed");
    return 0;
}

extern "C" int pf_fg_status_reset(void *ws, void *stream) {
    if (!ws) return fail(PF_EINVAL, "pf_fg_status_reset: null workspace");
    return launch_zero_fill(ws, FG_STATUS_WORDS * sizeof(unsigned), (hipStream_t)stream);
}
