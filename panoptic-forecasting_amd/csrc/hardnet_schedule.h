// The schedule of an inference forward (hardnet_schedule.cpp, host only): the plan's op table as a flat list of launches, every
// fusion and kernel choice made, every argument filled.  hardnet_plan.hip enqueues it; pf_debug_hardnet_schedule hands it to tests.
#pragma once
#include <vector>

#include "hardnet_plan.h"

namespace pf {

// Each kind names exactly one kernel.  S_CONV: inside build_schedule only, a convolution whose kernel is picked once the formats are known
enum StepKind : uint8_t {
    S_RANGE_CHECK, S_STEM, S_STEM_FRONT, S_PAIR, S_CONV, S_CONV_S4, S_CONV_S4_SHARE, S_CONV_S4_ADD, S_CONV_S4_TAIL, S_CONV_S4_DOWN, S_CONV_S4_LO, S_CONV_GENERIC, S_CONV_SPLIT, S_CONV_SPLIT1, S_CONV_WAVE, S_CONV_DMA,
    S_POOL, S_UPSAMPLE, S_HEAD };
struct PlainArgs { const float *src; float *dst; int planes, hin, win, hout, wout; size_t n; unsigned *status, *slot; };   // pool, upsample, range check
struct Step {
    StepKind kind;
    int op;          // first op of the table the step executes
    char tag[96];    // pf_profile_* label of its launches (empty unless the plan tags ops)
    // convolutions (and the front end's output) in the format decision: ranges [sb, se) read, destination, whether the kernel can
    // read / write the S4 layout (can_write: whatever it reads; can_write_s4: only when it reads S4 itself)
    int ci, need, sb, se;   // op whose weights it runs; need: bit 1 = even tile rows (pooling epilogue), bit 2 = fused stage
    uint32_t src_t[kConvMaxSrc], dst_t;
    bool can_read, can_write, can_write_s4;
    ConvDecision dec;   // decide_conv: its conv_s4 shape if it reads S4, else dec.ch = its fp32-source kernel (once picked: the launched shape)
    union {
        ConvArgs c; PairArgs pair; PlainArgs x;
        struct { StemArgs stem; FrontArgs front; char front_tag[96]; } sf;
        struct { HeadArgs h; float *orig; size_t orig_bytes; } head;
    } u;
};
inline bool is_conv_step(StepKind k) { return k >= S_CONV_S4 && k <= S_CONV_DMA; }

// One forward of plan p on B inputs of H x W: the fused stem's inputs (`stem`, pf_bg_forward) or a dense input (`dense_x`), the head's
// outputs, the workspace.  Computes with the pointers it is given and reads nothing through them.  fmt: per tensor 1 = S4, 0xFF / 0xFE =
// elided (pf_plan::last_fmt)
int build_schedule(const pf_plan *p, const StemArgs *stem, const float *dense_x, int B, int H, int W, int out_h, int out_w,
                   void *out_seg, int out_seg_is_i64, float *out_logits, float *out_orig, void *ws, size_t ws_bytes,
                   std::vector<Step> &steps, std::vector<uint8_t> &fmt);

}  // namespace pf
