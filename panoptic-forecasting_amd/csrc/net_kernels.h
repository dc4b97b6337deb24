// Non-GEMM stages of the bg network — interface.  stem_kernels.hip: what builds the network input; head_kernels.hip: upsample + argmax and
// the fused validation loss; resample_kernels.hip: pool and upsample; net_select.cpp (host only): which kernel a launch runs, its grid,
// LDS size and profile label - the launchers enqueue what it says, tests read it through pf_debug_net_choice without a device.
#pragma once
#include "pf_common.h"

namespace pf {

typedef float f32x4v __attribute__((ext_vector_type(4)));

struct StemArgs {
    const void *seg;       // [B,T,H,W] u8 or i64
    const float *depth;    // [B,T,H,W]
    const uint8_t *mask;   // [B,T,H,W] (ignored with PF_HOP_DEPTH_U16)
    const float *w;        // folded OIHW [16][T*(n_cls+1)][3][3]
    const float *wdep;     // depth-channel columns re-packed [tap][t][16] (uniform 64-B rows for scalar loads)
    const float *woh;      // one-hot rows re-packed [tap][t][n_cls + 1][16], last row of each group zero (nullable)
    const float *bias;     // [16]
    const uint8_t *lut;    // [256] id -> trainId (device)
    float *dst;            // [B,16,Hout,Wout] fp32, or (dst_fmt = 1) the packed-pair layout [B][2][4][Hout][Wout][4] fp16 of conv_mfma.h
    int dst_fmt;           // 1: only the 2x2-outputs-per-lane kernel writes it (choose_stem: family STEM_V4)
    float depth_mean, depth_std, min_depth, max_depth;
    int seg_is_i64, hop, B, T, n_cls, H, W, Hout, Wout;
    unsigned *status;      // range guard of the operand split (conv_mfma.h): |output| > 65504 raises PF_STATUS_RANGE; nullable
    unsigned *range_slot;  // ... and max |output| goes to this word of the status block (low side of the guard); nullable
    long long *probe;      // PF_PROBE builds only
};

struct HeadArgs {
    const float *logits;  // [B,C,Hin,Win]
    void *out_seg;        // [B,Hout,Wout] u8 or i64
    float *out_logits;    // nullable [B,C,Hout,Wout]
    int out_is_i64, B, C, Hin, Win, Hout, Wout;
};

int launch_stem(const StemArgs &a, hipStream_t s);
// status / slot (nullable): max |output| of the launch for the low side of the range guard (conv_mfma.h)
int launch_avgpool2(const float *src, float *dst, int planes, int Hin, int Win, unsigned *status, unsigned *slot, hipStream_t s);
int launch_upsample(const float *src, float *dst, int planes, int Hin, int Win, int Hout, int Wout, unsigned *status, unsigned *slot, hipStream_t s);
int launch_head(const HeadArgs &a, hipStream_t s);

// ---- tile shapes the kernels and the selector share
constexpr int kStemRow = 16;                 // floats per one-hot weight row in LDS (20 = conflict-free for any label mix; measured no faster: warped label maps are coherent)
constexpr int kHeadTH = 16, kHeadTW = 256;   // output tile of seg_loss_tile_kernel
constexpr int kHeadCH = 32, kHeadCW = 256;   // output tile of head_col_kernel
constexpr size_t kHeadLdsMax = 60 * 1024;    // dynamic LDS a tiled head / loss launch may ask for (its kernels' attribute is raised to it)

// ---- the built instantiations: X(variant index, template arguments...).  The selector makes each one's profile label from its row and
// the launchers their kernel tables, so an instantiation and its label are written once.
// v4 <3, HOP_D, HOP_LUT, FAST_DIV>, variant = HOP_D * 4 + HOP_LUT * 2 + FAST_DIV (the reciprocal division exists under the depth hop only)
#define PF_STEM_V4_INSTANCES(X) \
    X(0, false, false, false) X(2, false, true, false) X(4, true, false, false) X(5, true, false, true) X(6, true, true, false) X(7, true, true, true)
// v3 <3, SEG64, HOP_D, HOP_LUT>, variant = SEG64 * 4 + HOP_D * 2 + HOP_LUT
#define PF_STEM_V3_INSTANCES(X) \
    X(0, false, false, false) X(1, false, false, true) X(2, false, true, false) X(3, false, true, true) \
    X(4, true, false, false) X(5, true, false, true) X(6, true, true, false) X(7, true, true, true)
// class counts head_col_kernel<C> and seg_loss_tile_kernel<C> are built for
#define PF_HEAD_CLASSES(X) X(11) X(19)

// ---- net_select.cpp: the decisions.  Pure integer / fp32 host arithmetic, no HIP call, nothing allocated.
enum StemFamily { STEM_GENERIC = 0, STEM_V3 = 1, STEM_V4 = 2 };
struct StemChoice {
    int family, variant;                     // StemFamily; row of the family's instance list (0 for the generic kernel)
    bool seg64, hop_d, hop_lut, fast_div;    // the template arguments in force (v3: no fast_div, v4: no seg64, generic: run-time flags)
    dim3 grid;                               // 256 lanes per workgroup, one output each on 64 x 4; v4: 2 x 2 outputs each, 128 x 8
    size_t lds;                              // the one-hot weight rows: 9 taps x T x (n_cls + 1) rows of kStemRow floats
    const char *label;
};
constexpr unsigned kNetBlock = 256;          // lanes per workgroup of every kernel here
// workgroups of a grid-stride kernel over `total` items
static inline unsigned grid_for(size_t total) {
    size_t g = (total + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}
// PF_OK, or PF_EUNSUPPORTED: the weights exceed the LDS budget; dst_fmt = 1 with a kernel that writes fp32 only
int choose_stem(const StemArgs &a, StemChoice *c);
int stem_family(const StemArgs &a);          // the family alone: the schedule fuses the front end behind STEM_V4 only (dst_fmt = 1)
// is  q = x * r;  q += fma(-q, std, x) * r  (r = 1 / std in fp32) the correctly rounded x / std for every x the in-register depth hop
// can produce?  (gates FAST_DIV; cached for the last parameter set)
bool stem_fast_div_exact(float mean, float stdv, float dmin, float dmax);

enum HeadKind { HEAD_PLAIN = 0, HEAD_QUAD = 1, HEAD_TILED = 2 };   // head_kernel, head4_kernel, head_col_kernel<C>
struct HeadChoice { int kind; dim3 grid; size_t lds; const char *label; };
HeadChoice choose_head(const HeadArgs &a);

struct LossChoice {
    dim3 grid;                               // seg_loss_tile_kernel<C>: one workgroup per kHeadTH x kHeadTW output tile and image
    size_t blocks, ws_bytes, lds;            // workgroups = partial sums of three doubles; the workspace that holds them; dynamic LDS
    const char *label;
};
// PF_OK, or PF_EUNSUPPORTED: C is not built (nothing filled); the source window of a tile does not fit LDS (grid, blocks, ws_bytes filled)
int choose_seg_loss(int B, int C, int Hin, int Win, int Hout, int Wout, LossChoice *c);
void seg_loss_geometry(int B, int Hout, int Wout, LossChoice *c);   // grid, blocks and ws_bytes alone (they depend on the output size only)

}  // namespace pf
