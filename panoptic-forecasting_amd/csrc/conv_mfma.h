// Direct (implicit-GEMM) fp32 convolution on the gfx950 matrix cores — interface.
//
// Replaces the ATen/cuDNN convolutions behind reference hardnet.py:16-25 (ConvLayer = conv + BN + ReLU,
// BN folded into weight/bias) for 3x3 (stride 1/2, pad 1) and 1x1 kernels, reading the HarDBlock
// "concatenation" (hardnet.py:225-230) as up to four channel ranges of earlier tensors instead of a
// torch.cat copy.
#pragma once
#include "conv_pack.h"
#include "pf_blob.h"
#include "pf_common.h"

namespace pf {

struct ConvArgs {
    const float *src[kConvMaxSrc];   // base of each source tensor [B, ctotal, Hin, Win]
    int src_ctotal[kConvMaxSrc];     // channels of the tensor the range lives in
    int src_choff[kConvMaxSrc];      // first channel of the range inside that tensor
    int src_cstart[kConvMaxSrc + 1]; // prefix sums of range lengths (conv input channel numbering)
    int src_chunk0[kConvMaxSrc + 1]; // first K chunk of each range ([n_src] = nchunks) in the launched kernel's chunk
                                     // size; every range is padded to whole chunks: a chunk never straddles tensors
    int n_src;
    const float *wpk;  // packed weights in the layout of the launched kernel family (conv_pack.h)
    const float *bias; // [n_tiles_total*16], zero padded
    float *dst;        // [B, dst_ctotal, Hout, Wout]
    int dst_ctotal, dst_choff;
    int Cin, Cout, Hin, Win, Hout, Wout;
    int tilesX, tilesY, nchunks, relu;
    // fast path (conv_dma.hip) only:
    const float *zero_page;  // >= 16 B of zeros (source of out-of-image / padding DMA pieces)
    int ntiles;              // ceil(Cout/16)
    // fused epilogue stages (conv_epilogue.h); zero-initialised = plain conv
    int no_bias;             // skip the bias add (the low-resolution half of a commuted upsample+1x1 conv)
    int pool;                // 2x2 average pool in the epilogue: dst is [B, dst_ctotal, Hout/2, Wout/2]
    const float *res;        // residual [B, res_ctotal, Hres, Wres], bilinearly upsampled (align_corners) and added
    int res_ctotal, res_choff, Hres, Wres;
    float res_sh, res_sw;    // (Hres-1)/(Hout-1), (Wres-1)/(Wout-1)
    int res_lds_off;         // float offset of the staged residual window in the kernel's LDS, or -1: sample from memory
    int res_rows, res_cols;  // conv_s4 1x1: fixed window size per channel (upper bounds of what a tile touches)
    unsigned res_magic_cs, res_magic_cols;   // ... and 2^32 / d + 1 of its channel stride and its columns (lane index -> element)
    const float *wrem;       // conv_dma remainder path: weights of the last `rem` couts, [chunk][kgroup][tap][RV][4 ch]
    int rem;                 // > 0: couts handled on the vector ALU; ntiles then counts FULL 16-cout tiles only
    int src_begin, src_end;      // input ranges to accumulate (whole conv: 0, n_src)
    int chunk_begin, chunk_end;  // = src_chunk0[src_begin], src_chunk0[src_end] (filled at launch)
    long long *probe;        // PF_PROBE builds only: in-kernel timestamps of workgroup 0 / wave 0 (else nullptr)
    unsigned *status;        // range guard of the two-term operand split (below): word 0 of the forward's workspace, or
                             // nullptr (fp32-only plans, training): epilogues OR PF_STATUS_RANGE into it when they store |v| > 65504
    unsigned *range_slot;    // ... and keep max |v| of what this launch stored here (low side of the guard, below); nullable
    int kacc;                // conv_dma 3x3 (training forward): per-round partial sums added into a second accumulator set (blocked summation)
    int accum;               // fp32 NCHW stores of conv_mfma.hip and of epi_store (conv_dma / conv_wave): dst += result (gradient
                             // accumulation of the training path); not combined with rem / pool / S4 destinations
    float acc_scale;         // split kernels (conv_split.hip, conv_s4.hip) only: their weights are packed as fp16 terms of
                             // w * 2^k (k per conv, split_weight_scale()); the raw sums are multiplied by 2^-k (exact)
    // ---- packed-pair ("S4") activation layout, conv_s4.hip: a tensor of C channels is stored as
    //      [B][2 terms: hi, mid][C4 = ceil(C/4)][H][W][4] fp16 with x ~= hi + mid (split_terms() below): the same
    //      4 B per element as fp32 and exactly the two terms the split kernels feed the matrix pipe with
    int dst_fmt;             // 0: fp32 NCHW, 1: S4 (epi_store / epi_store_pooled of conv_epilogue.h)
    int dst_c4;              // channel groups of the dst tensor
    int dst_limit;           // S4: stores cover buffer channels [dst_choff, dst_limit) = dst_choff + Cout, rounded up to a
                             // whole group when this conv also zero-fills the tail of its last group
    int src_fmt;             // 1: every source is S4 (conv_s4 kernels only)
    int src_c4[kConvMaxSrc];      // channel groups of each source tensor
    int src_g0[kConvMaxSrc];      // first group a range touches = src_choff / 4
    int src_gn[kConvMaxSrc];      // number of groups it touches
    int src_ent0[kConvMaxSrc + 1];// first K entry of each range ("group entries": one group of one range; padded per range to
                                  // whole rounds when the conv was packed with pad_sources)
    // ---- the share / add forms of the 3x3 packed-pair kernel (conv_s4.hip: launch_conv_s4_share / _add; zero for every other launch).
    //      An odd HarDBlock layer P = conv(S) and its consumer C = conv(P ++ S ++ others): the share launch runs over S with P's rows
    //      and C's rows over S in common cout tiles, the add launch runs C over its other ranges and adds the stored sums
    float *share;            // [B][ceil(share_cout / 4)][H][W][4] fp32: C's sums over S times C's acc_scale (no bias, no ReLU)
    int share_off;           // share form: first matrix row of C's part = P's couts rounded up to 4
    int share_cout;          // C's output channels
    float share_scale;       // share form: C's acc_scale (this launch's acc_scale is P's)
    // ---- the fold forms (conv_s4.hip: launch_conv_s4_tail / _down; zero for every other launch): this launch L is a 3x3 conv whose slice
    //      is read last by a 1x1 conv R.  L's finished values, still in registers as the two terms R would read back, are multiplied by
    //      R's weights together with the centre pixels of R's other channels (read from their packed planes), so R's launch goes away.
    //      R's operands, the same for every form:
    const float *fold_w;     // pack_conv_weights_fold(): R's A fragments, [cout tile][chunk 0: R's other channels, chunk 1 (, 2): this launch's couts][term][64 lanes][8 fp16]
    const float *fold_bias;  // R's bias, zero padded to whole tiles
    float fold_scale;        // R's acc_scale
    const float *fold_src;   // R's other channels: the packed tensor they live in, fold_c4 channel groups (term stride = fold_c4 planes), ...
    int fold_c4, fold_g0, fold_gn;   // ... its groups fold_g0 .. fold_g0 + fold_gn - 1 (fold_gn <= 8: one K = 32 chunk; 0: none)
    //      tail: R has no ReLU and at most 16 couts and goes to fp32 NCHW; it is linear in its input and the slice's only reader, so the
    //      slice is never stored
    //      lo (three cout tiles): as tail with up to 64 couts of R; the slice is stored as by the plain form unless dst is nullptr
    float *tail_dst;         // R's destination [B, tail_ctotal, Hout, Wout] fp32, R's couts from channel tail_choff on
    int fold_cout, tail_ctotal, tail_choff;   // fold_cout: R's couts, whatever the form (tail: <= 16, down, lo: <= 64, down3: <= 96)
    //      down (down3: three cout tiles, up to 96 couts of R): R has a ReLU, up to 64 couts and a 2x2 average pool behind it.  The slice is stored as by the plain form; R's pooled
    //      output is stored as packed pairs, or as fp32 where its readers want that
    float *down_dst;         // R's pooled destination: down_fmt = 1, the S4 layout [B][2 terms][down_c4][Hout / 2][Wout / 2][4] fp16 ...
    int down_c4, down_choff, down_limit;   // ... its channel groups, R's first channel in it and the dst_limit of R's stores;
    int down_fmt, down_ctotal;             // down_fmt = 0: fp32 [B, down_ctotal, Hout / 2, Wout / 2], R's couts from channel down_choff on
    unsigned *down_status, *down_slot;     // range guard of the pooled values: the status word and slot of R's destination (nullable)
};

// ---- the two-term operand split of conv_split.hip / conv_s4.hip ------------------------------------------------------
// Every fp32 operand x of a convolution is fed to the 16-bit matrix pipe as x ~= hi + mid with TWO fp16 TERMS, both
// rounded to nearest even:
//     hi = fp16_rne(x),  mid = fp16_rne(x - hi)          (x - hi is exact in fp32)
// Operand bound (proved in tests/test_host_logic.py::test_split_operand_bound by exhausting every fp32 exponent, checked
// bit for bit against the device in tests/test_gpu_conv.py::test_s4_layout_round_trip): |x - hi| <= half an fp16 ulp of x,
// so the residual needs at most 12 significand bits below hi's last one and mid (11 bits, nearest) leaves
//     |x - hi - mid| <= 2^-23 |x|                      for 2^-2 <= |x| <= 65504   (fp32's own rounding: 2^-24)
//     |x - hi - mid| <= 2^-25  (half an fp16 subnormal step: absolute)   for |x| < 2^-2
// against 2^-21 |x| for the round-toward-zero pair of round 2 and 2^-17 |x| for a pair of bf16 terms, at the same storage,
// the same instruction rate (v_mfma_f32_16x16x32_f16) and the same three products hi*hi + hi*mid + mid*hi; the dropped
// product mid*mid is <= 2^-22 of a product.  The price is fp16's range:
//   * activations: |x| > 65504 cannot be represented.  It is never silent: every kernel that produces a tensor a split
//     kernel may read (the conv epilogues, the stem, the layout packer) compares what it stores against 65504 and raises
//     bit PF_STATUS_RANGE of the forward's status word (ConvArgs::status = word 0 of the workspace; range_acc / range_commit
//     below); the caller re-runs that forward on the fp32 matrix instructions or fails (pfhip.h: pf_hardnet_status,
//     bg_model.py: on_range_overflow).  FC-HarDNet activations behind folded BatchNorm are O(1..100);
//   * weights: packed on the host (round to nearest even) after an exact per-conv scaling by 2^k that puts max|w| into
//     [2^14, 2^15) - small weights keep both terms in fp16's normal range - and the kernels multiply their raw sums
//     by 2^-k (ConvArgs::acc_scale) before the bias: exact, so the scaling is invisible in the result.
// v_mfma_f32_16x16x32_f16 multiplies fp16 subnormals exactly (measured: tools/ubench/f16_split.hip).
typedef _Float16 split_t;
typedef split_t split_x2 __attribute__((ext_vector_type(2)));
typedef split_t split_x4 __attribute__((ext_vector_type(4)));
typedef split_t split_x8 __attribute__((ext_vector_type(8)));
constexpr float kSplitMaxAbs = 65504.f;   // largest |x| the pair represents (to 2^-23)
// two values at a time: {hi0, hi1}, {mid0, mid1}.  hi: v_cvt_pk_f16_f32 (gfx950) rounds to nearest even, two values per issue.
// mid = fp16(x - hi): one mixed-precision FMA per value (v_fma_mixlo / mixhi_f16: hi read as fp16, x as fp32, the fp32 difference
// - exact - rounded to nearest even into one half of the result register) - 3 instructions per pair where convert back, subtract,
// convert takes 5; the same bits (tests/test_gpu_conv.py::test_s4_layout_round_trip pins the device's patterns to the host's)
__device__ __forceinline__ void split_terms2(float x0, float x1, split_x2 &hi, split_x2 &mid) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    hi = __builtin_convertvector(f32x2{x0, x1}, split_x2);
    const unsigned hu = __builtin_bit_cast(unsigned, hi);
    unsigned mu;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(mu) : "v"(hu), "v"(x0));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(mu) : "v"(hu), "v"(x1));
    mid = __builtin_bit_cast(split_x2, mu);
#endif
}
// range guard: m = running max |v| of what a lane stores; one compare + (never taken) branch at the end.  NaN cannot arise
// from finite guarded inputs (products <= 65504 * 2^15, K <= a few thousand: the fp32 accumulators cannot overflow)
// (two v_max3_f32 with |.| source modifiers; written with fmaxf / fabsf hipcc quiets every input first: 7 instructions)
__device__ __forceinline__ float range_acc(float m, float a, float b, float c, float d) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(m) : "v"(a), "v"(b));
    asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(m) : "v"(c), "v"(d));
#endif
    return m;
}
// Low side of the same guard.  Below |x| = 2^-2 the pair keeps an ABSOLUTE 2^-25 (mid is an fp16 subnormal), so a tensor
// whose values are all tiny loses relative precision where the reference's fp32 Conv2d (hardnet.py:16-25) does not.  Two
// measures (hardnet_plan.hip): every tensor channel is stored multiplied by a power of two chosen at plan creation so that
// its expected magnitude is kRangeTarget (exact re-parameterisation of the folded weights: producers' rows * s, consumers'
// columns / s), and every launch that produces a split operand reports the maximum |v| of what it stored to its own word of
// the forward's status block (ConvArgs::range_slot); range_finalize_kernel raises PF_STATUS_RANGE_LOW when a launch's
// reported maximum is below kRangeLowMax: the unflagged operand bound is then |x - hi - mid| <= 2^-23 |x| + 2^-25, with
// 2^-25 <= 2^-19 max|tensor| - and the caller re-runs a flagged forward on the fp32 matrix instructions as for overflow.
// Only a SAMPLE of a launch's workgroups reports (range_sampled: 8-15 of them, picked by a hash of the workgroup id):
// agent-scope atomics on one address execute memory-side at ~10 ns each (measured: every wave of a 16 384-workgroup launch
// reporting tripled the kernel's time, and a cached pre-check of the word does not help - the XCD L2s keep serving the value
// from before the atomics).  Sampling is conservative for this test: a tensor whose values are ALL below the threshold is
// below it on every sample, so it is always flagged; a tensor with larger values escapes the flag as soon as one sampled
// workgroup stored one (8 x 32 pixels x all its output channels each).  A reporting wave ORs 1 into the bit pattern, so a word
// of 0 means "no report" (an op without a slot) and a word of 1 "every sampled value was exactly zero": neither is low - exact
// zeros lose nothing in the pair (a dead-ReLU layer, blank frames); the flag needs a NON-ZERO maximum below kRangeLowMax.
constexpr float kRangeTarget = 8.0f;          // expected magnitude of a stored channel after the plan's scaling
constexpr float kRangeLowMax = 0.015625f;     // 2^-6: a launch whose reported max |v| is below it raises PF_STATUS_RANGE_LOW
__device__ __forceinline__ bool range_sampled() {   // uniform per workgroup
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned total = gridDim.x * gridDim.y * gridDim.z;
    const unsigned id = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const unsigned mask = total >= 16u ? (1u << (28 - __builtin_clz(total))) - 1u : 0u;   // keeps one workgroup in 2^floor(log2(total)) / 8
    return (((id * 0x9E3779B1u) >> 9) & mask) == 0u;
#else
    return false;
#endif
}
// m = max |v| over what the lane stored (>= 0; v_max3 drops NaN); lanes that have exited are simply not counted
__device__ __forceinline__ void range_commit(unsigned *status, unsigned *slot, float m) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (status == nullptr) return;
    if (!(m <= kSplitMaxAbs)) atomicOr(status, 1u);   // PF_STATUS_RANGE
    if (slot == nullptr || !range_sampled()) return;
    // wave maximum by a scalar walk over the lanes that exceed the running value (~5 steps for unordered data)
    const unsigned mb = __builtin_bit_cast(unsigned, m);
    unsigned wm = 0;
    unsigned long long above = __builtin_amdgcn_ballot_w64(mb > wm);
    while (above != 0) {
        wm = (unsigned)__builtin_amdgcn_readlane((int)mb, (int)__builtin_ctzll(above));
        above = __builtin_amdgcn_ballot_w64(mb > wm);
    }
    const unsigned lane_id = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    if (lane_id == (unsigned)__builtin_ctzll(__builtin_amdgcn_ballot_w64(true))) atomicMax(slot, wm | 1u);   // first active lane
#endif
}
template <typename V4>   // any 4-float vector type
__device__ __forceinline__ void split_terms4(const V4 &v, split_x4 &hi, split_x4 &mid) {
    split_x2 h0, m0, h1, m1;
    split_terms2(v[0], v[1], h0, m0);
    split_terms2(v[2], v[3], h1, m1);
    hi = split_x4{h0[0], h0[1], h1[0], h1[1]};
    mid = split_x4{m0[0], m0[1], m1[0], m1[1]};
}
#define PF_MFMA_SPLIT(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)
// (host side, weight packing: split_host_f16 / split_host_f32 / split_weight_scale of conv_pack.h)

// Workgroup -> (pixel tile, cout group) for the grids dim3(pixel tiles, cout groups, B) of the fast kernels.  Workgroups are
// dispatched in linear id order (x fastest) to the 8 XCDs round-robin, and each XCD has its own L2.  With a tile count that
// is a multiple of 8, id % 8 names the XCD and id / 8 the position in that XCD's queue; the queue is laid out as
//     XCD x  <-  a contiguous band of tiles;  consecutive positions = the cout groups of ONE tile, then the next tile
// so that (a) the halo rows / partially used 128-B lines neighbouring tiles share and (b) the whole input tile that the
// cout groups of a tile share (a 1x1 conv with Cout = 119 at NT = 2 is four workgroups reading the same pixels) are read
// from HBM once and then from that XCD's L2.  In plain (x, y) order the cout groups of a tile are a whole image of
// workgroups apart and every one of them streams the input from HBM again.
__device__ __forceinline__ void xcd_tile_order(int ntiles_xy, int &tile_lin, int &group) {
#if defined(__HIP_DEVICE_COMPILE__)
    if ((ntiles_xy & 7) != 0) {
        tile_lin = (int)blockIdx.x;
        group = (int)blockIdx.y;
        return;
    }
    const int ngroups = (int)gridDim.y;
    const int lin = (int)blockIdx.x + ntiles_xy * (int)blockIdx.y;
    const int xcd = lin & 7, pos = lin >> 3;
    const int t = pos / ngroups;
    group = pos - t * ngroups;
    tile_lin = xcd * (ntiles_xy >> 3) + t;
#endif
}

// Tiling choice for one conv (depends on shape only; fixed at plan time for the weight packing).
struct ConvTiling {
    int ks, stride;
    int kc;   // input channels staged per LDS chunk (multiple of 4)
    int nt;   // 16-wide cout tiles per workgroup
    int twt;  // workgroup tile width in 16-pixel units (4: 4x64, 2: 8x32, 1: 16x16 pixels)
    int cout_blocks, nchunks;
    size_t packed_floats() const;   // of pack_conv_weights (conv_pack.cpp)
};

ConvTiling choose_tiling(int ks, int stride, int cin, int cout, int wout_hint);
// Enqueue one conv for a batch of B images (generic path: any stride/width).
int launch_conv(const ConvArgs &a, const ConvTiling &t, int B, hipStream_t stream);

// Fast path (Win % 4 == 0): a.wpk must point at pack_conv_weights_tiled() output and
// a.nchunks = ceil(Cin / kc) with kc = dma_kc(ks, stride) input channels per double-buffered stage.
constexpr int dma_kc_ct(int ks, int stride) { return ks == 1 ? 16 : (stride == 2 ? 4 : 8); }
inline int dma_kc(int ks, int stride) { return dma_kc_ct(ks, stride); }
// conv_dma's vector-ALU cout path: the last `rem` (1..16) output channels; accumulators rv in {2,4,8,12,16} >= rem
inline int dma_rem_rv(int rem) { return rem <= 2 ? 2 : (rem + 3) / 4 * 4; }
// how many trailing output channels of a 3x3/s1 conv go to the vector ALU (0 = none): the partial tile
inline int dma_valu_split(int cout) {
    if (cout < 16) return 0;
    return cout % 16;
}
// force_wm/force_nt > 0 override the cost model (tuning runs); model_B > 0: the cost model sees this batch size
// instead of B (batch-invariant shape choice, plan option "table_batch")
int launch_conv_dma(const ConvArgs &a, int ks, int stride, int B, hipStream_t stream, int force_wm = 0, int force_nt = 0, int model_B = 0);
// the shape (*wm, *nt) launch_conv_dma picks for these arguments; whether it has a kernel for it (residual window: at launch only)
bool conv_dma_supported(const ConvArgs &a, int ks, int stride, int B, int force_wm, int force_nt, int model_B, int *wm, int *nt);

// Wave-autonomous path (conv_wave.hip; stride 1, Win % 4 == 0): a.wpk must point at pack_conv_weights_wave()
// output and a.nchunks = ceil(Cin / wave_kc(ks)).  Tile = mh rows x 16 pixels, nt cout tiles, wk-way K split.
constexpr int wave_kc_ct(int ks) { return ks == 1 ? 32 : 8; }
inline int wave_kc(int ks) { return wave_kc_ct(ks); }
int launch_conv_wave(const ConvArgs &a, int ks, int mh, int nt, int wk, int B, hipStream_t stream);
bool conv_wave_supported(const ConvArgs &a, int ks, int mh, int nt, int wk);   // launch_conv_wave has a kernel for this launch
// LDS bytes of a conv_wave workgroup (WaveCfg in conv_wave.hip asserts the match)
constexpr size_t wave_lds_bytes(int ks, int mh, int nt, int wk) {
    const int kc = wave_kc_ct(ks), ih = mh + ks - 1, iw = 16 + (ks == 3 ? 8 : 0);
    const int raw = ih * iw, plane = (raw + 15) / 32 * 32 + 16, nit = (kc * (plane / 4) + 63) / 64;
    const size_t ring = (size_t)wk * 2 * nit * 256, red = (size_t)wk * mh * nt * 256;
    return 4 * (ring > red ? ring : red);
}

// split path (conv_split.hip; 3x3/s1, Wout % 4 == 0, no fused epilogue; two fp16 terms per operand, see split_terms2
// above): a.wpk must point at pack_conv_weights_split() output, chunks of 8 channels, a.acc_scale = 1 / the weights' scale.
int launch_conv_split(const ConvArgs &a, int nt, int wide, int B, hipStream_t stream);
bool conv_split_supported(const ConvArgs &a);   // launch_conv_split has a kernel for this launch
// 1x1/s1 on the same scheme (chunks of 32 channels; pack_conv_weights_split1()); supports the fused epilogue stages
int launch_conv_split1(const ConvArgs &a, int nt, int B, hipStream_t stream);
bool conv_split1_supported(const ConvArgs &a, int nt);   // ... and launch_conv_split1 (a residual window must fit LDS)

// S4 path (conv_s4.hip, 1x1: conv_s4_1x1.hip; stride 1, W % 4 == 0): every source in the packed-pair layout, tiles arrive by LDS-DMA, no split
// phase; a.wpk = pack_conv_weights_s4() output (conv_pack.h: its K order).
struct S4Range { int choff, ch; };   // a source range in the channel numbering of its tensor
struct KOrder;   // the ranges of a launch in K order with their starts in the conv's input-channel numbering (conv_ranges.h, which counts
                 // the entries and rounds): they may be packed in ANOTHER order than the one they are concatenated in (conv_pair.hip)
// the pixel tile a 3x3 launch is asked for: 8x32, 8x64, 16x32 on 8 waves, 8x32 with 2 / 4 wave groups splitting the rounds.  The values
// are the ABI of pf_debug_force_conv(5, nt, tile, 0) and the contents of conv_s4_tuned.inc
enum S4Tile : int { S4_8x32 = 0, S4_8x64 = 1, S4_16x32 = 2, S4_8x32_K2 = 3, S4_8x32_K4 = 4 };
// The instantiation that runs a request of nt cout tiles per workgroup on `tile` for a conv of ntiles cout tiles and `rounds` K rounds
// (conv_select.cpp; 1x1 and kacc - the blocked sums of training - know 8x32 only): conv_s4[_blocked]_kernel<NT, TW, TH, KS>,
// conv_s4_1x1_kernel<NT, *>.  The schedules resolve when they make the step; launch_conv_s4 dispatches on the result
struct S4Shape { int NT, TW, TH, KS; };
S4Shape s4_resolve(int ks, int nt, int tile, int ntiles, int rounds, bool kacc);
int launch_conv_s4(const ConvArgs &a, int ks, const S4Shape &shape, int B, hipStream_t stream);
// a pair P = conv3x3(S), C = conv3x3(P ++ S ++ others) as two launches that read S once (8 x 32 tiles, nt cout tiles per workgroup;
// ConvArgs::share ..): `share` = P's launch whose matrix also holds C's rows over S and stores their sums, `add` = C's launch over its
// other ranges, which adds them.  share_wanted (conv_select.cpp): mode = the plan's share_s option (0 never, 1 the measured rule, 2 wherever
// the forms exist)
int launch_conv_s4_share(const ConvArgs &a, int nt, int B, hipStream_t stream);
int launch_conv_s4_add(const ConvArgs &a, int nt, int B, hipStream_t stream);
inline int share_row0(int p_cout) { return (p_cout + 3) / 4 * 4; }   // a lane's four couts never straddle the two convs
bool share_wanted(int p_cin, int p_cout, int c_cin, int c_cout, int h, int w, int B, int mode);
// the fold forms: a 3x3 launch L of two or three cout tiles - all in one workgroup - on 8 x 32 tiles that also computes the 1x1 conv R
// reading its slice last (ConvArgs::fold_..).  tail: R without ReLU, one cout tile, into fp32 (ConvArgs::tail_..); R's output is stored
// instead of L's slice.  down: R with ReLU, at most kDownTiles cout tiles, and the 2x2 average pool behind it (ConvArgs::down_..); L's
// slice is stored too.  The wide forms, L of three cout tiles (<3, 32, 8, 1>): down3 = down with at most kWideTiles cout tiles of R;
// lo: R = the low-resolution half of a commuted upsample + 1x1 conv (no bias, no ReLU, at most kLoTiles cout tiles) into the fp32
// scratch its other half samples (ConvArgs::tail_..); L's slice is stored unless R is its only reader (ConvArgs::dst == nullptr).
// tail_wanted / down_wanted / lo_wanted (conv_select.cpp): mode = the plan's fold_final / fold_down / fold_lo option (0 never, 1 the
// measured rule, 2 wherever the form exists); cin, cout = the 3x3 conv's, r_cout = R's
enum FoldForm : int { FOLD_TAIL, FOLD_DOWN, FOLD_DOWN3, FOLD_LO };
constexpr int kFoldForms = 4;
int launch_conv_s4_tail(const ConvArgs &a, int B, hipStream_t stream);
int launch_conv_s4_down(const ConvArgs &a, int B, hipStream_t stream);   // (two or three cout tiles: by a.ntiles)
int launch_conv_s4_lo(const ConvArgs &a, int B, hipStream_t stream);
bool tail_wanted(int cin, int cout, int r_cout, int h, int w, int B, int mode);
bool down_wanted(int cin, int cout, int r_cout, int h, int w, int B, int mode);
bool lo_wanted(int cin, int cout, int r_cout, int h, int w, int B, int mode);
// K = 32 chunks of R's A fragments: R's other channels (at most 8 groups), then the launch's first 32 couts (a lane's 4 + 4 values of
// cout tiles 0 and 1); the wide forms: a third chunk whose low half is the lane's 4 values of cout tile 2, zeros above them
constexpr int kTailChunks = 2, kWideChunks = 3;
constexpr int kDownTiles = 4;    // the down form's fragments hold this many cout tiles of R, zeros past R's couts
constexpr int kWideTiles = 6, kLoTiles = 4;   // ... and the wide forms' (down3, lo)
constexpr int kDownFragBytes = kDownTiles * kTailChunks * 2 * 64 * 16;
constexpr int kWideFragBytes = kWideTiles * kWideChunks * 2 * 64 * 16;   // (room for either wide form in the stage ring)
inline size_t fold_packed_floats(int ntiles, int chunks = kTailChunks) { return (size_t)ntiles * chunks * 2 * 64 * 4; }

// conv_pair.hip: an odd HarDBlock layer P = conv3x3(S) computed inside its consumer C = conv3x3(P ++ S ++ others) (hardnet.py:177-194)
struct PairArgs {
    ConvArgs c;              // the consumer; sources in the K order [S, other ranges.., P's output] (the last one is never read from
                             // memory: src_ent0 / nchunks describe it, its src pointer is unused), weights packed in that order with
                             // pad_sources = 1 and P's range declared as {0, p_cout}
    const float *p_wpk;      // P: pack_conv_weights_pair_p() of its single range: [tile][round][instr 0, instr 1] blocks ...
    const float *p_w9;       // ... and the ninth tap [tile][round][term][64 lanes][4 fp16] (lane group 0 / 1 = the round's entries); bias zero padded
    const float *p_bias;
    float p_acc_scale;
    float *p_dst;            // P's destination (packed pairs): its slice of the block's output tensor
    int p_dst_c4, p_dst_choff, p_dst_limit, p_cout, p_cin, p_ntiles, p_relu;
    unsigned *p_range_slot;  // max |v| of what P stored (range guard, low side); nullable
    int rounds_s;            // rounds of S = P's rounds = C's first rounds
    int round_d;             // C's first round over P's planes
    int merged;              // 1: c.wpk was packed from C's weights WITH P's weights in rows 4 .. 4 + p_cout - 1 of C's last cout tile
                             // (columns of S only; each conv's own 2^k): P's values at the tile's own pixels come out of C's matrix
                             // instructions, conv_pair computes P only on the halo ring.  Needs roundup4(C cout) + P cout <= 16 * tiles
};
bool conv_pair_supports(int c_cout, int p_cout);
bool conv_pair_merged_supports(int c_cout, int p_cout);     // PairArgs::merged possible for these channel counts?
// conv_select.cpp: run this pair as one conv_pair launch?  mode = the plan's fuse_pairs option (1: where measured / modelled faster, 2: wherever possible,
// 3: wherever possible and never merged, 4: the merged pairs only)
bool pair_wanted(int p_cin, int p_cout, int c_cin, int c_cout, int h, int w, int B, int mode);
int launch_conv_pair(const PairArgs &pa, int B, hipStream_t stream);
// s4_layout.hip: layout conversion (tests, tensor taps), fp32 NCHW <-> S4, and the range guard's own kernels
// status (nullable, device): PF_STATUS_RANGE is raised when an element exceeds what the pair represents (|x| > 65504)
int launch_s4_pack(const float *src, void *dst, int B, int C, int H, int W, unsigned *status, hipStream_t stream);
// raises PF_STATUS_RANGE in *status if any of the n floats at x is not |x| <= 65504 (NaN included); max |x| -> *slot (nullable)
int launch_range_check(const float *x, size_t n, unsigned *status, unsigned *slot, hipStream_t stream);
// status block of a forward's workspace (hardnet_plan.hip): word 0 = published PF_STATUS_* bits of the last forward, word
// sticky_word = OR over all forwards since the host cleared it, word live_word = what the running forward's kernels OR into,
// words first_slot .. + n_slots - 1 = reported max |v| per launch (bit patterns), the next n_slots words = those of the last forward
int launch_range_finalize(unsigned *st, int live_word, int first_slot, int n_slots, int sticky_word, hipStream_t stream);
int launch_s4_unpack(const void *src, float *dst, int B, int C, int H, int W, hipStream_t stream);

// Fused front end (conv_front.hip): 3x3 stride-1 conv (16 -> 24 channels) + 3x3 stride-2 conv (24 -> <= 32) in one kernel; the
// input is the stem output in the packed-pair layout, the tensor between the two convs stays in LDS
struct FrontArgs {
    const void *x;          // stem output, packed pairs [B][2][4][H1][W1][4] fp16
    const void *w1, *w2;    // pack_conv_weights_s4() of the two convs (already scaled by 2^k)
    const float *bias1, *bias2;   // zero padded to 32
    float scale1, scale2;   // 2^-k
    float *dst;             // [B][dst_ctotal][H2][W2] fp32 or packed pairs
    int dst_fmt, dst_c4, dst_ctotal, dst_choff, dst_limit;
    int H1, W1, H2, W2, C1, C2, relu1, relu2;
    int tilesX, tilesY;     // strips x vertical segments (set by the launcher)
    int seg_steps;          // steps (2 output rows each) per segment (set by the launcher)
    unsigned *status;
    unsigned *range_slot_mid, *range_slot;   // max |v| of the tensor between the two convs / of the output (low side of the range guard); nullable
    long long *probe;       // PF_PROBE builds only (tools/probe_front.py), else nullptr
};

bool conv_front_supports(int c0, int c1, int c2, int h1, int w1, int dst_ctotal);
int launch_conv_front(const FrontArgs &a, int B, hipStream_t s);

// Kernel / shape choice for one stride-1 conv (conv_select.cpp).  The values are the ABI of pf_debug_force_conv and the contents of
// conv_tuned.inc / conv_s4_tuned.inc (3 was conv_valu: the whole 3x3 conv on v_pk_fma_f32, measured and removed - DESIGN.md 3.2)
enum ConvKind : int { CONV_AUTO = 0, CONV_DMA = 1, CONV_WAVE = 2, CONV_SPLIT = 4, CONV_S4 = 5 };
// four ints (the table rows aggregate-initialise it); what p0..p2 mean per kind is said by the makers and readers only
struct ConvChoice {
    int kind, p0, p1, p2;
    static ConvChoice dma(int wm = 0, int nt = 0) { return {CONV_DMA, wm, nt, 0}; }   // 0: by conv_dma's cost model
    static ConvChoice wave(int mh, int nt, int wk) { return {CONV_WAVE, mh, nt, wk}; }
    static ConvChoice split(int nt, int wide) { return {CONV_SPLIT, nt, wide, 0}; }   // wide = 1: 8x64-pixel tiles
    bool is(ConvKind k) const { return kind == k; }   // (CONV_S4: S4 sources, NT and S4Tile; table rows and the forced choice only)
    int dma_wm() const { return p0; }
    int dma_nt() const { return p1; }
    int wave_mh() const { return p0; }
    int wave_nt() const { return p1; }
    int wave_wk() const { return p2; }
    int split_nt() const { return p0; }
    int split_wide() const { return p1; }
    int s4_nt() const { return p0; }
    int s4_tile() const { return p1; }
};
// need: bit 1 = even tile rows if conv_wave is chosen (pooling epilogue)
ConvChoice choose_conv(int ks, int stride, int cin, int cout, int hout, int wout, int B, int need = 0, int use_tuned = 1);
// conv_s4 table row, if any: CONV_S4 with its shape, or CONV_AUTO = the fp32-source kernel measured faster in situ
bool choose_s4(int ks, int cin, int cout, int hout, int wout, int B, ConvChoice *out);
// Everything the schedules decide about one conv from its shape, the plan's options and the forced choice
struct ConvQuery {
    int ks, stride, cin, cout, hout, wout;
    int B;          // the batch the choice is made for (option "table_batch")
    int need;       // bit 1 = even tile rows (pooling epilogue), bit 2 = another fused stage
    bool generic;   // input width % 4 != 0: the generic kernel, nothing to choose
    bool has_split, has_s4;   // the plan packed the conv's weights for conv_split / conv_s4
    bool use_tuned, split_f16, kacc;   // options "use_tuned_table", "split_f16"; blocked sums (training)
    int rounds;     // K rounds of the S4 packing
    ConvChoice force;   // conv_force()
};
struct ConvDecision {
    ConvChoice ch;      // its fp32-source kernel (CONV_AUTO: generic)
    bool wants_s4;      // S4 sources if the plan can give them to it ...
    int s4_nt, s4_tile; // ... then conv_s4 is asked for this shape ...
    S4Shape s4;         // ... and runs this one
};
ConvDecision decide_conv(const ConvQuery &q);
long long *probe_buffer();
// tuning hook (pf_debug_force_conv): CONV_AUTO = automatic
ConvChoice conv_force();
inline bool conv_forced() { return !conv_force().is(CONV_AUTO); }
inline bool force_allows_s4() { return !conv_forced() || conv_force().is(CONV_S4); }
// pf_debug_force_conv(1, wm > 0, nt, 0): the conv_dma shape of every convolution of a training step
inline bool forced_dma_shape(int *wm, int *nt) {
    const ConvChoice f = conv_force();
    if (!f.is(CONV_DMA) || f.dma_wm() <= 0) return false;
    *wm = f.dma_wm(); *nt = f.dma_nt();
    return true;
}

}  // namespace pf
