// Convolutions on activations stored PRE-SPLIT ("S4" layout, conv_mfma.h): the operand-split scheme of conv_split.hip without its
// memory side.
//
// conv_split.hip reads fp32 NCHW, and every consumer of a tensor splits it again: per round of 8 channels a thread holds 32
// staging registers, spends 15-20 % of the round on conversions + 8 ds_write_b128 and needs two barriers because the
// activation buffer cannot be overwritten while it is read (profiles/r02_experiments.md: the memory side and the matrix
// side of a 91->28 layer need 285 and 318 us alone and 406 us together).  Here the PRODUCER's epilogue writes
//     [B][2 terms: hi, mid][C4 = ceil(C/4)][H][W][4 channels] fp16       hi = fp16(x), mid = fp16(x - hi)
// - the same 4 B per element as fp32 and exactly what these consumers feed the matrix pipe with, so nothing is lost for
// them - and a consumer's halo tile arrives by LDS-DMA (buffer_load_dwordx4 ... lds, 16 B = 2 pixels x 4 channels of one
// term; out-of-image pieces carry an out-of-range offset and land as zeros = the convolution's padding): no staging
// registers, no conversion, no LDS stores, double-buffered stages with ONE barrier per round.
//
// Channel groups of 4 (not 8): FC-HarDNet's tensors have 10/18/28/46 channels; a range is read as the groups it touches
// (weights of channels it does not own inside its first/last group are zero), so 10 channels cost 12, not 16.  A block's
// concatenated output tensor is one buffer: layers write their slice (4-B granularity: all offsets are even) and whoever
// reads the whole block reads no padding at all.
//
// 3x3: GEMM view as in conv_split.hip (M = 16 pixels of a row, N = 16 couts, K = 32 = 4 lane groups x 8 values), a lane's 8
// K-values = the 4 channels of TWO group entries for one tap: two ds_read_b64 per term.  A round = 2 entries = 8 channels.
// Nine taps do not fill whole instructions of 4 tap slots (conv_split.hip and the first version of this kernel spent 12
// slots on them: a quarter of the matrix instructions multiplied zeros, and with the memory side out of the way these
// kernels are bound by the matrix pipe - profiles/r02_experiments.md).  Here a round issues TWO full instructions
//     instr 0: (0,0) (0,1) | (1,0) (1,1)        instr 1: (2,0) (2,1) | (0,2) (1,2)
// (the two lane groups one ds_read_b64 pass serves read the same tile row - conflict-free for any row pitch - except the
// last pair, a 2-way conflict on one pass) and the ninth tap (2,2) is COLLECTED: in round r only lane group r & 3 reads
// its (2,2) fragments, into registers that survive the round; after four rounds the four lane groups hold the K-slices
// of four different rounds and one more instruction (weights packed to match) retires them: 9 instructions per 4 rounds
// instead of 12, no zero slots.  Wave w DMAs plane (term = w >> 1, entry = w & 1) of a stage.
// 1x1 (conv_s4_1x1.hip): K = 32 = 8 group entries per instruction and round; 8x32-pixel tiles, the fused epilogue stages of
// conv_epilogue.h.  This file: the 3x3 forms (conv_s4_kernel.inc), their launchers and launch_conv_s4, which dispatches to both.
#include <cstring>

#include "conv_s4.h"
#include "pf_prof.h"

#ifndef PF_PROBE
#define PF_PROBE 0
#endif
#if PF_PROBE   // shader-clock stamps of one workgroup in the middle of the grid (tools/probe_s4.py)
#define S4_PROBE(i) do { if (threadIdx.x == 0 && blockIdx.x == gridDim.x / 2 && blockIdx.y == 0 && blockIdx.z == gridDim.z / 2 && a.probe && (i) < 60) a.probe[i] = clock64(); } while (0)
#else
#define S4_PROBE(i) do { } while (0)
#endif

// the DMA parts of the next stage go out after MFMA groups 1, 3, .. of a round (every placement measured within 1 %)
[[maybe_unused]] constexpr int kS4IssueFirst = 1, kS4IssueStep = 2;

namespace pf {

// KS_ = 2 / 4 (the small levels, 64x128 and below at B = 16: a few hundred workgroups of 20-50 dependent rounds on 256 CUs):
// KS_ wave groups per workgroup on the same pixel tile, each with its own stage ring; group k runs the k-th part of the rounds
// (parts of a multiple of 4 rounds: the collected tap spans groups of 4); groups 1.. hand their sums over through LDS and
// group 0 runs the epilogue.  KS_ times the waves per tile and 1 / KS_ of the dependent chain per wave.
template <int NT, int TW_, int TH_ = 8, int KS_ = 1>
struct S4Cfg {
    static constexpr int TW = TW_, TH = TH_, MTR = TW / 16, MP = 2 * MTR;   // TH / 2 waves x MP M-tiles = TH rows x TW pixels
    static constexpr int KS = KS_;
    static constexpr int NW = TH / 2, NTHR = 64 * NW;                       // per wave group.  TH = 16: 8 waves share the stage (half the weight bytes per MAC, halo 1.27 instead of 1.41)
    static constexpr int IW = TW + 4, IH = TH + 2;                        // halo tile, 2-pixel apron left/right (16-B pieces)
    static constexpr int ROWP = IW / 2, PIECES = IH * ROWP;               // 16-B pieces per (term, entry) plane
    static constexpr int NDMA_ALL = (PIECES + 63) / 64;                   // DMA instructions per plane ...
    static constexpr int NDMA = (NDMA_ALL + NW / 4 - 1) / (NW / 4);       // ... of which a wave issues this many (NW / 4 waves per plane)
    // COLREG (the <2, 32> and <3, 32> shapes): the collected-tap block (a third of a flush round's weights, used once in four
    // rounds) does NOT pass through LDS - its fragments are loaded straight into registers right before the flush products -
    // and the planes hold exactly their pieces: 38.5 instead of 48 KB (NT = 2) / 46.5 instead of 60 KB (NT = 3) per workgroup
    // = 4 instead of 3 / 3 instead of 2 workgroups per CU, with the register count capped by the launch bounds (128: 6 values,
    // 168: 8 values parked in scratch across the main loop).  Resident waves are what these kernels are short of
    // (profiles/r02_experiments.md: taking one workgroup per CU away costs 16-52 %; giving one: -3.6 % / -14 %).  The other
    // shapes cannot reach their next workgroup this way (<1, 32> would need 102 registers: 16 spills in the main loop, +35 %;
    // <4, 32> and the 8x64 shapes stay at 2) and keep the third block in LDS, where it costs no exposed load
    static constexpr bool COLREG = (NT == 2 || NT == 3) && TW_ == 32;
    static constexpr int PLANE = COLREG ? PIECES * 16 : NDMA_ALL * 64 * 16;   // bytes (lanes past the last piece are masked off)
    static constexpr int ABUF = 4 * PLANE;                                // [term][entry] per stage
    static constexpr int WBLK = 2 * 64 * 16;                              // one instruction's weights of one cout tile: [term][lane][8 fp16]
    static constexpr int BPT = COLREG ? 2 : 3;                            // blocks per cout tile in LDS: instr 0, instr 1[, collected tap]
    static constexpr int WBUF = NT * BPT * WBLK;                          // [nt][block][term][lane]
    static constexpr int WPIECES = WBUF / 16, NITW = (WPIECES + NTHR - 1) / NTHR;
    static constexpr size_t STAGES_BYTES = 2 * (size_t)ABUF + 2 * (size_t)WBUF;
    static constexpr size_t LDS_BYTES = KS * STAGES_BYTES + NT * 16 * sizeof(float);   // + the bias values of the workgroup's couts
    static_assert(KS == 1 || (size_t)MP * NT * NW * 64 * 16 <= STAGES_BYTES, "the K-split hand-over uses group 1's stage ring");
};

// KACC (training, train_s4.hip): every round's products (72 terms per output: 8 channels x 9 taps) are summed on their own and added
// to a second accumulator set - blocked summation, like the fp32 step's conv_dma (KACC there) and like ATen - instead of one fp32
// chain over all 9 Cin terms: the forward pass of a training step is then as close to float64 as the fp32 step's
#define S4_KERNEL_NAME conv_s4_kernel
#define S4_KERNEL_KACC 0
#define S4_KERNEL_EPI 0
#define S4_KERNEL_WAVES (KS_ == 4 ? 1 : (TH_ == 16 || KS_ == 2) ? 2 : (TW_ == 32 && NT <= 2) ? 4 : (TW_ == 32 && NT == 3) ? 3 : 2)
#include "conv_s4_kernel.inc"
#undef S4_KERNEL_NAME
// the share / add forms (an odd HarDBlock layer's launch also sums its consumer's rows over their common source; the consumer's launch
// adds them: launch_conv_s4_share / _add below), instantiated for 8 x 32 tiles without a K split at the plain form's launch bounds
#undef S4_KERNEL_EPI
#define S4_KERNEL_NAME conv_s4_share_kernel
#define S4_KERNEL_EPI 1
#include "conv_s4_kernel.inc"
#undef S4_KERNEL_NAME
#undef S4_KERNEL_EPI
#define S4_KERNEL_NAME conv_s4_add_kernel
#define S4_KERNEL_EPI 2
#include "conv_s4_kernel.inc"
#undef S4_KERNEL_NAME
#undef S4_KERNEL_EPI
// the fold forms (the launch also computes the 1x1 conv that reads its slice last: launch_conv_s4_tail / _down below), instantiated for
// two cout tiles - down and lo: also, or only, for three - on 8 x 32 tiles without a K split at the plain form's launch bounds.  tail: the
// 1x1 conv's output is stored, the slice not
#define S4_KERNEL_NAME conv_s4_tail_kernel
#define S4_KERNEL_EPI 3
#include "conv_s4_kernel.inc"
#undef S4_KERNEL_NAME
#undef S4_KERNEL_EPI
// down: the slice is stored, and the 2x2 average pool of the 1x1 conv's output
#define S4_KERNEL_NAME conv_s4_down_kernel
#define S4_KERNEL_EPI 4
#include "conv_s4_kernel.inc"
#undef S4_KERNEL_NAME
#undef S4_KERNEL_EPI
// lo (three cout tiles): the 1x1 conv is the low-resolution half of a commuted upsample + 1x1 conv; the slice is stored if anyone else reads it
#define S4_KERNEL_NAME conv_s4_lo_kernel
#define S4_KERNEL_EPI 5
#include "conv_s4_kernel.inc"
#undef S4_KERNEL_NAME
#undef S4_KERNEL_EPI
#undef S4_KERNEL_KACC
#undef S4_KERNEL_WAVES
// the blocked-sum form (instantiated for 8 x 32 tiles without a K split): one workgroup per CU fewer than the plain form where the
// second accumulator set needs the registers
#define S4_KERNEL_NAME conv_s4_blocked_kernel
#define S4_KERNEL_KACC 1
#define S4_KERNEL_EPI 0
#define S4_KERNEL_WAVES (NT == 1 ? 4 : (NT == 2 ? 3 : 2))
#include "conv_s4_kernel.inc"
#undef S4_KERNEL_NAME
#undef S4_KERNEL_KACC
#undef S4_KERNEL_EPI
#undef S4_KERNEL_WAVES

// one launcher for the seven forms of the 3x3 kernel (conv_s4_kernel.inc); the label = the symbol rocprofv3 reports (bench.py looks
// its PMC bytes up by it)
enum S4Form { S4_PLAIN, S4_BLOCKED, S4_SHARE, S4_ADD, S4_TAIL, S4_DOWN, S4_LO };
constexpr const char *kS4FormName[] = {"conv_s4_kernel", "conv_s4_blocked_kernel", "conv_s4_share_kernel", "conv_s4_add_kernel", "conv_s4_tail_kernel", "conv_s4_down_kernel",
                                       "conv_s4_lo_kernel"};
template <S4Form FORM, int NT, int TW_, int TH_, int KS_>
static constexpr auto s4_kernel() {   // (only the form asked for is instantiated)
    if constexpr (FORM == S4_PLAIN) return &conv_s4_kernel<NT, TW_, TH_, KS_>;
    else if constexpr (FORM == S4_BLOCKED) return &conv_s4_blocked_kernel<NT, TW_, TH_, KS_>;
    else if constexpr (FORM == S4_SHARE) return &conv_s4_share_kernel<NT, TW_, TH_, KS_>;
    else if constexpr (FORM == S4_ADD) return &conv_s4_add_kernel<NT, TW_, TH_, KS_>;
    else if constexpr (FORM == S4_TAIL) return &conv_s4_tail_kernel<NT, TW_, TH_, KS_>;
    else if constexpr (FORM == S4_DOWN) return &conv_s4_down_kernel<NT, TW_, TH_, KS_>;
    else return &conv_s4_lo_kernel<NT, TW_, TH_, KS_>;
}
template <S4Form FORM, int NT, int TW_ = 32, int TH_ = 8, int KS_ = 1>
static int launch_s4_form(const ConvArgs &a0, int B, hipStream_t s) {
    using C = S4Cfg<NT, TW_, TH_, KS_>;
    constexpr auto kernel = s4_kernel<FORM, NT, TW_, TH_, KS_>();
    constexpr const char *name = kS4FormName[FORM];
    ConvArgs a = a0;
    a.tilesX = (a.Wout + C::TW - 1) / C::TW;
    a.tilesY = (a.Hout + C::TH - 1) / C::TH;
    static bool attr_set = false;
    if (!attr_set) {
        PF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS_BYTES));
        attr_set = true;
    }
    char label[96];
    snprintf(label, sizeof(label), "void pf::%s<%d, %d, %d, %d>(pf::ConvArgs)", name, NT, TW_, TH_, KS_);
    const double px = (double)B * a.Hout * a.Wout;
    // share: the matrix instructions also produce the consumer's rows, stored as fp32 sums in groups of 4; add: reads them
    const int rows = FORM == S4_SHARE ? a.Cout + a.share_cout : a.Cout;
    const double sums = FORM == S4_SHARE || FORM == S4_ADD ? (double)(a.share_cout + 3) / 4 * 4 : 0.0;
    // folds: both convs' flops; read the 3x3 conv's input and the other channels of the 1x1 conv's.  tail writes the 1x1 conv's output only,
    // down its slice and a quarter of the 1x1 conv's pixels, lo the 1x1 conv's output and the slice if it is stored
    constexpr bool FOLD = FORM == S4_TAIL || FORM == S4_DOWN || FORM == S4_LO;
    const double flops = 2.0 * px * rows * a.Cin * 9 + (FOLD ? 2.0 * px * a.fold_cout * (4 * a.fold_gn + a.Cout) : 0.0);
    const double stored = FORM == S4_TAIL ? (double)a.fold_cout : FORM == S4_DOWN ? a.Cout + 0.25 * a.fold_cout
                          : FORM == S4_LO ? (a.dst ? a.Cout : 0) + (double)a.fold_cout : a.Cout + sums;
    const double extra = FOLD ? px * 4 * a.fold_gn + (double)a.fold_cout * (4 * a.fold_gn + a.Cout) : 0.0;
    ProfScope ps(s, label, flops, 4.0 * ((double)B * a.Cin * a.Hin * a.Win + px * stored + (double)rows * a.Cin * 9 + extra));
    hipLaunchKernelGGL(kernel, dim3(a.tilesX * a.tilesY, (a.ntiles + NT - 1) / NT, B), dim3(C::NTHR * C::KS), C::LDS_BYTES, s, a);
    PF_LAUNCH_CHECK(name);
    return PF_OK;
}

// a pair P = conv3x3(S), C = conv3x3(P ++ S ++ others) as two launches that read S once:
// share: a = P's launch with a.wpk = pack of [P's rows; zero rows up to a.share_off; C's rows over the columns of S] (a.ntiles tiles of
//        that matrix), a.share / share_off / share_cout / share_scale filled; P's slice is stored as by the plain kernel
// add:   a = C's launch without the range S (weights packed without its columns), a.share / share_cout filled
// what every form but the plain one asks of its launch: packed sources and slice, stride 1, no fused epilogue stage (share / add:
// allow_share - the scratch tensor is theirs), the whole K range
static int check_s4_form(const ConvArgs &a, const char *who, bool allow_share) {
    if (!a.src_fmt || !a.dst_fmt) return fail(PF_EINVAL, "%s: sources and destination in the S4 layout only", who);
    if ((a.Wout & 3) != 0 || a.Hin != a.Hout || a.Win != a.Wout) return fail(PF_EUNSUPPORTED, "%s: stride 1, width %% 4 == 0 only", who);
    if (a.pool || a.res || a.no_bias || a.kacc || (a.share && !allow_share))
        return fail(PF_EUNSUPPORTED, "%s: no fused epilogue stages of its own", who);
    if (a.chunk_begin != 0 || a.chunk_end != a.nchunks) return fail(PF_EUNSUPPORTED, "%s: whole K range only", who);
    return PF_OK;
}
static int check_share(const ConvArgs &a, const char *who) {
    if (int rc = check_s4_form(a, who, true)) return rc;
    if (!a.share || a.share_cout < 1 || (reinterpret_cast<uintptr_t>(a.share) & 15) != 0) return fail(PF_EINVAL, "%s: no scratch tensor", who);
    return PF_OK;
}
#define PF_S4_SHARE(FORM_) \
    nt = nt < 1 ? 1 : (nt > a.ntiles ? a.ntiles : nt); \
    if (nt == 1) return launch_s4_form<FORM_, 1>(a, B, s); \
    if (nt == 2) return launch_s4_form<FORM_, 2>(a, B, s); \
    return launch_s4_form<FORM_, 3>(a, B, s);
int launch_conv_s4_share(const ConvArgs &a, int nt, int B, hipStream_t s) {
    if (int rc = check_share(a, "conv_s4 share")) return rc;
    if ((a.share_off & 3) != 0 || a.share_off < a.Cout || a.share_off + a.share_cout > a.ntiles * 16)
        return fail(PF_EINVAL, "conv_s4 share: rows %d + %d in %d tiles", a.share_off, a.share_cout, a.ntiles);
    PF_S4_SHARE(S4_SHARE)
}
int launch_conv_s4_add(const ConvArgs &a, int nt, int B, hipStream_t s) {
    if (int rc = check_share(a, "conv_s4 add")) return rc;
    if (a.share_cout != a.Cout) return fail(PF_EINVAL, "conv_s4 add: stored sums of %d channels for %d", a.share_cout, a.Cout);
    PF_S4_SHARE(S4_ADD)
}
#undef PF_S4_SHARE
// the fold forms: a = the 3x3 conv's plain launch with R's operands (a.fold_..: fragments, bias and scale, the planes of R's other channels,
// R's couts, at most max_cout) and the form's destination of R filled; ntiles: the cout tiles of the instantiation that will run
static int check_fold(const ConvArgs &a, const char *who, int max_cout, int ntiles = 2) {
    if (int rc = check_s4_form(a, who, false)) return rc;
    if (a.ntiles != ntiles) return fail(PF_EUNSUPPORTED, "%s: %d cout tiles, the form is built for %d", who, a.ntiles, ntiles);
    if (!a.fold_w || !a.fold_bias || a.fold_cout < 1 || a.fold_cout > max_cout || a.fold_gn < 0 || a.fold_gn > 8 || (a.fold_gn && !a.fold_src) ||
        (reinterpret_cast<uintptr_t>(a.fold_w) & 15) != 0 || (reinterpret_cast<uintptr_t>(a.fold_bias) & 15) != 0 || a.fold_g0 < 0 ||
        a.fold_g0 + a.fold_gn > a.fold_c4)
        return fail(PF_EINVAL, "%s: second conv of %d couts over %d groups", who, a.fold_cout, a.fold_gn);
    return PF_OK;
}
int launch_conv_s4_tail(const ConvArgs &a, int B, hipStream_t s) {
    if (int rc = check_fold(a, "conv_s4 tail", 16)) return rc;
    if (!a.tail_dst || a.tail_choff < 0 || a.tail_choff + a.fold_cout > a.tail_ctotal)
        return fail(PF_EINVAL, "conv_s4 tail: second conv of %d couts over %d groups", a.fold_cout, a.fold_gn);
    return launch_s4_form<S4_TAIL, 2>(a, B, s);
}
int launch_conv_s4_down(const ConvArgs &a, int B, hipStream_t s) {
    const bool wide = a.ntiles == 3;
    if (int rc = check_fold(a, "conv_s4 down", 16 * (wide ? kWideTiles : kDownTiles), wide ? 3 : 2)) return rc;
    if (a.Hout < 2 || a.Wout < 2) return fail(PF_EUNSUPPORTED, "conv_s4 down: nothing to pool at %d x %d", a.Hout, a.Wout);
    const bool packed_ok = (a.down_choff & 1) == 0 && a.down_limit >= a.down_choff + a.fold_cout && a.down_limit <= 4 * a.down_c4 &&
                           a.down_limit <= (a.down_choff + a.fold_cout + 3) / 4 * 4;
    if (!a.down_dst || a.down_choff < 0 || (a.down_fmt ? !packed_ok : a.down_choff + a.fold_cout > a.down_ctotal))
        return fail(PF_EINVAL, "conv_s4 down: pooled destination of %d channels from %d (limit %d) in %d groups", a.fold_cout, a.down_choff, a.down_limit, a.down_c4);
    return wide ? launch_s4_form<S4_DOWN, 3>(a, B, s) : launch_s4_form<S4_DOWN, 2>(a, B, s);
}
int launch_conv_s4_lo(const ConvArgs &a, int B, hipStream_t s) {
    if (int rc = check_fold(a, "conv_s4 lo", 16 * kLoTiles, 3)) return rc;
    if (!a.tail_dst || a.tail_choff < 0 || a.tail_choff + a.fold_cout > a.tail_ctotal)
        return fail(PF_EINVAL, "conv_s4 lo: second conv of %d couts over %d groups", a.fold_cout, a.fold_gn);
    return launch_s4_form<S4_LO, 3>(a, B, s);
}

// a.wpk = pack_conv_weights_s4() output, a.nchunks = s4_rounds(), a.src_fmt = 1 (sources in the S4 layout, a.src_c4 /
// src_g0 / src_ent0 filled), a.chunk_begin/chunk_end = the rounds to run.
// sh = s4_resolve() of the request (the schedules keep it in the step): the instantiations below are all it can name
int launch_conv_s4(const ConvArgs &a, int ks, const S4Shape &sh, int B, hipStream_t s) {
    if (!a.src_fmt) return fail(PF_EINVAL, "conv_s4: sources are not in the S4 layout");
    if ((a.Wout & 3) != 0 || a.Hin != a.Hout || a.Win != a.Wout) return fail(PF_EUNSUPPORTED, "conv_s4: stride 1, width % 4 == 0 only");
    if (ks == 3) {
        if (a.pool || a.res || a.no_bias) return fail(PF_EUNSUPPORTED, "conv_s4 3x3: no fused epilogue stages");
        if (a.chunk_begin != 0 || a.chunk_end != a.nchunks) return fail(PF_EUNSUPPORTED, "conv_s4 3x3: whole K range only");
#define PF_S4(FORM_, NT_, TW_, TH_, KS_) \
    if (sh.NT == NT_ && sh.TW == TW_ && sh.TH == TH_ && sh.KS == KS_) return launch_s4_form<FORM_, NT_, TW_, TH_, KS_>(a, B, s);
        if (a.kacc) {   // blocked summation (training)
            PF_S4(S4_BLOCKED, 1, 32, 8, 1) PF_S4(S4_BLOCKED, 2, 32, 8, 1) PF_S4(S4_BLOCKED, 3, 32, 8, 1)
        } else {
            PF_S4(S4_PLAIN, 1, 32, 8, 1) PF_S4(S4_PLAIN, 2, 32, 8, 1) PF_S4(S4_PLAIN, 3, 32, 8, 1)
            PF_S4(S4_PLAIN, 4, 32, 8, 1)    // 4 cout tiles per pixel fragment read from LDS (2 workgroups per CU)
            PF_S4(S4_PLAIN, 1, 64, 8, 1) PF_S4(S4_PLAIN, 2, 64, 8, 1)
            PF_S4(S4_PLAIN, 1, 32, 16, 1) PF_S4(S4_PLAIN, 2, 32, 16, 1)   // 8 waves
            PF_S4(S4_PLAIN, 1, 32, 8, 2) PF_S4(S4_PLAIN, 2, 32, 8, 2)     // two wave groups split the rounds ...
            PF_S4(S4_PLAIN, 1, 32, 8, 4) PF_S4(S4_PLAIN, 2, 32, 8, 4)     // ... FOUR (16 waves on one tile)
        }
#undef PF_S4
    } else if (sh.TW == 32 && sh.TH == 8 && sh.KS == 1) {
        const bool fused = a.pool || a.res || a.no_bias;
#define PF_S41(NT_) \
    if (sh.NT == NT_) return fused ? launch_s41_cfg<NT_, 1>(a, B, s) : launch_s41_cfg<NT_, 0>(a, B, s);
        PF_S41(1) PF_S41(2) PF_S41(3) PF_S41(4)
#undef PF_S41
    }
    return fail(PF_EUNSUPPORTED, "conv_s4 %dx%d: shape <%d, %d, %d, %d> is not built", ks, ks, sh.NT, sh.TW, sh.TH, sh.KS);
}

}  // namespace pf
