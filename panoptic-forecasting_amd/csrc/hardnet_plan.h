// The inference plan as its translation units share it (not part of the ABI): plan_create.hip builds it (options, range
// normalisation, weight arena), hardnet_schedule.cpp turns a forward of it into a list of launches (hardnet_schedule.h),
// hardnet_plan.hip enqueues that list, plan_access.hip answers questions about it.
#pragma once
#include <vector>

#include "conv_epilogue.h"
#include "conv_ranges.h"
#include "net_kernels.h"
#include "pf_net.h"

// where the packings of one convolution start (floats into dev_weights).  Offset 0 is the zero page, never a packing: a packing
// the conv does not have is 0
struct ConvPlan {
    pf::ConvTiling tiling;
    size_t wpk_off = 0;
    size_t bias_off = 0;  // (padded to 16*n_tiles)
    size_t raw_off = 0;   // folded OIHW copy (stem only)
    size_t dep_off = 0;   // stem only: depth-channel columns [tap][t][16]
    size_t oh_off = 0;    // stem only: one-hot rows [tap][t][n_cls + 1][16] with a zero row per group
    size_t tiled_off = 0; // per-cout-tile packing for the DMA fast path
    int tiled_chunks = 0;
    size_t rem_off = 0;   // conv_dma vector-ALU cout weights (3x3/s1 convs, rem_count trailing couts)
    int rem_count = 0;
    size_t wave_off = 0;  // fragment-order packing for the wave-autonomous path (stride 1 only)
    int wave_chunks = 0;
    size_t split_off = 0; // fp16 hi/mid fragments for the split path (3x3/s1 and 1x1)
    int split_chunks = 0;
    size_t s4_off = 0;    // conv_s4.hip packing (stride-1 3x3 and 1x1)
    int s4_rounds = 0;
    bool s4_pad = false;  // its ranges padded to whole rounds (the conv may run one range at a time)
    size_t front_off = 0; // conv_s4-style packing of a 3x3 STRIDE-2 conv with one input range (second conv of conv_front.hip)
    float split_acc_scale = 1.0f;          // 2^-k: the split / S4 packings hold fp16 terms of w * 2^k (conv_mfma.h)
    // conv_pair.hip, kept on the CONSUMER (op i; its producer is op i - 1): the consumer's weights in the K order [S, others, P] with
    // every range padded to whole rounds, the producer's two-instruction stream and its ninth-tap stream
    size_t pair_c_off = 0, pair_two_off = 0, pair_nine_off = 0;
    int pair_rounds = 0;
    bool pair_merged = false;              // pair_c_off carries P's weights in C's padding rows (conv_mfma.h: PairArgs::merged)
    // the share / add launches of the same pair (conv_s4.hip), kept on the consumer too and packed only by plans created with share_s != 0:
    // [P's rows; C's rows over the columns of S] over S (share_a_tiles cout tiles), and C without the columns of S (share_b_rounds rounds)
    size_t share_a_off = 0, share_b_off = 0;
    int share_a_tiles = 0, share_b_rounds = 0;
    // the fold forms (conv_s4.hip; kFolds below), kept on the PRODUCER L (op i; the 1x1 conv R that reads its slice last is op i + 1) and
    // packed only by plans created with the form's option != 0: R's A fragments, an offset in floats into the form's region
    // (pf_plan::fold, whose first 64 floats are zeros: 0 = the op has none).  Regions of their own: the weight arena stays what it was
    // without the forms
    size_t fold_off[pf::kFoldForms] = {0, 0, 0, 0};
};

// The switches a plan carries (include/pfhip.h documents each), with their defaults.  g_plan_opt is the process-wide set
// (pf_set_option); plan creation copies all of it, pf_hardnet_plan_set_option changes the copy
struct PlanOptions {
    int fuse_pool = 1, fuse_upsample = 1, valu_remainder = 1, split_f16 = 1, use_tuned_table = 1;
    int table_batch = 0;       // > 0: per-layer kernel choice as if the batch were this (batch-invariant numerics); per plan only
    int fuse_front = 1;        // stem -> conv_front.hip (3x3 s1 + 3x3 s2 in one kernel, the tensor between them never stored)
    int range_guard = 1;       // kernels raise PF_STATUS_RANGE in the workspace's status word when they store |v| > 65504 while
                               // two-term fp16 operands are in use (conv_mfma.h); 0 = no checks (the clamp-free fp32 path needs none)
    int packed_acts = 1;       // tensors whose producers and consumers all support it live in the S4 layout (conv_s4.hip)
    int normalize_ranges = 1;  // per-channel power-of-two scaling of the stored activations, fixed at plan creation; process-wide only
    int profile_tag_ops = 0;   // pf_profile_* records carry one label per op of the table (tools/)
    int fuse_pairs = 1;        // conv_pair.hip: an odd HarDBlock layer runs inside its consumer where both read / write packed pairs (0 = two launches)
    int share_s = 1;           // conv_s4.hip share / add: an odd HarDBlock layer's launch also sums its consumer's rows over their common source
                               // (0 = off, and a plan created with 0 packs nothing for it; 1 = conv_select.cpp::share_wanted; 2 = wherever built)
    // conv_s4.hip folds: a 3x3 conv's launch also computes the 1x1 conv that reads its slice last (0 = off, and a plan created with 0 packs
    // nothing for the form; 1 = the form's rule in conv_select.cpp; 2 = wherever built).  The forms: kFolds below
    int fold_final = 1;        // tail: the 1x1 conv is small, goes to fp32 and is the slice's only reader; the slice is never stored
    int fold_down = 1;         // down: the 1x1 conv has a ReLU and a 2x2 average pool behind it, which the launch computes too; the slice is stored as ever
                               // (3x3 convs of two cout tiles, and - down3 - of three)
    int fold_lo = 1;           // lo: the 1x1 conv is the low-resolution half of a commuted upsample + 1x1 conv (fp32 scratch, no bias, no ReLU); the
                               // 3x3 conv has three cout tiles; its slice is stored only if something else reads it
};

struct pf_plan {
    pf::NetTable net;
    std::vector<ConvPlan> conv;  // parallel to net.ops
    std::vector<int> readers;    // per tensor: number of ops that read it
    float *dev_weights = nullptr;
    uint8_t *dev_lut = nullptr;
    size_t dev_floats = 0;
    struct FoldRegion {
        std::vector<float> host;    // the form's packings (ConvPlan::fold_off), empty when the plan has none ...
        float *dev = nullptr;       // ... and their upload
    } fold[pf::kFoldForms];
    PlanOptions opt;             // read only by forwards of this plan
    // formats of the last forward (pf_hardnet_tensor_read): 1 = S4, 0xFF = elided (never stored: conv_front.hip), 0xFE = its last
    // slice elided (never stored: the tail and lo forms of conv_s4.hip)
    mutable std::vector<uint8_t> last_fmt;
    // range normalisation (conv_mfma.h): tensor t, channel c is stored multiplied by chan_scale[t][c] (a power of two; 1 for
    // the network input, the head's input and every tensor no convolution reads); inv_scale_off[t] = offset in dev_weights
    // of the reciprocals (pf_hardnet_tensor_read), or 0 when all are 1
    std::vector<std::vector<float>> chan_scale;
    std::vector<size_t> inv_scale_off;
    std::vector<uint8_t> feeds_conv;   // per tensor: a convolution reads it (directly or through pool / upsample ops)
};

namespace pf {

extern PlanOptions g_plan_opt;

// workspace: PF_WS_STATUS_BYTES of status words - word 0 = PF_STATUS_* bits of the last forward (written once, by the
// range_finalize launch that ends a forward), word 1 = the same bits ORed over every forward since the host cleared it
// (sticky), word 2 = the word the kernels of the running forward OR their flags into, words kSlot0 + i = max |v| that op i
// of the table reported so far (bit pattern; low side of the range guard, conv_mfma.h), words kSlot0 + kMaxSlots + i = the
// same for the last finished forward (pf_hardnet_range_maxima).  The finalizer leaves word 2 and the live slots cleared for
// the next forward: the host zeroes the block once (pf_hardnet_status_reset) and no forward starts with a memset.  Then
// every tensor except the network input in its own 256-B aligned region
constexpr size_t kStatusBytes = PF_WS_STATUS_BYTES;
constexpr int kStickyWord = PF_WS_STICKY_OFFSET / 4, kLiveWord = 2, kSlot0 = 16, kMaxSlots = ((int)(kStatusBytes / 4) - kSlot0) / 2;

// the plan's geometry for a batch of B inputs of H x W: every tensor's size and workspace offset ((size_t)-1: not stored), and
// the workspace size (hardnet_schedule.cpp: the schedule's first pass).  share_off (nullable): offset of the scratch region of the share / add launches - one region,
// sized for the largest pair the plan has packings for, reused by all of them; (size_t)-1 when the plan has none
int layout(const pf_plan *p, int B, int H, int W, std::vector<Dims> &d, std::vector<size_t> &off, size_t &total, size_t *share_off = nullptr);

// ops i (P) and i + 1 (C) form a pair conv_pair.hip can run as one launch (plan_create.hip)
bool is_conv_pair(const NetTable &t, size_t i);
// What distinguishes the fold forms (FoldForm: conv_mfma.h).  Common to all: L = op i, a 3x3 stride-1 conv of l_tiles cout tiles; R = the
// 1x1 stride-1 conv behind it, whose range ends with L's slice: op i + 1 and its single range, or (up) op i + 2 and the range of the
// upsample op i + 1 between them, whose whole output is R's first range of two (hardnet_plan.hip runs that range at the low resolution)
struct FoldDesc {
    int l_tiles;                    // L's cout tiles: two, or three (the wide forms: a third K chunk in R's fragments)
    bool r_relu;                    // R's ReLU
    int r_tiles;                    // R's cout tiles at most = the tiles its fragments are packed as
    bool pool;                      // op i + 2 is R's 2x2 average pool and the only reader of R's output
    bool up;                        // op i + 1 is an upsample of the range, R = op i + 2 reads all of its output first
    bool other_readers;             // ops other than R may read L's slice (it is stored)
    int PlanOptions::*option;
    bool (*wanted)(int cin, int cout, int r_cout, int h, int w, int B, int mode);
    constexpr int chunks() const { return l_tiles == 3 ? kWideChunks : kTailChunks; }
    constexpr size_t r_at() const { return up ? 2 : 1; }   // R = op i + r_at()
};
constexpr FoldDesc kFolds[kFoldForms] = {
    {2, false, 1, false, false, false, &PlanOptions::fold_final, tail_wanted},      // FOLD_TAIL
    {2, true, kDownTiles, true, false, true, &PlanOptions::fold_down, down_wanted},   // FOLD_DOWN
    {3, true, kWideTiles, true, false, true, &PlanOptions::fold_down, down_wanted},   // FOLD_DOWN3
    {3, false, kLoTiles, false, true, true, &PlanOptions::fold_lo, lo_wanted},        // FOLD_LO
};
// ops i (L) and i + r_at() (R) have the form: conv_s4.hip can compute R in L's launch (plan_create.hip)
bool is_conv_fold(const NetTable &t, size_t i, FoldForm form);
// Host only (the pf_debug_* entries; plan_create.hip): the plan this blob would give now under the process-wide options, nothing
// uploaded - `host` = its weight arena, dev_weights and the fold regions' dev stay null.  who: the caller's name in error messages
int debug_plan(const char *who, const void *blob, size_t bytes, int in_ch, int n_cls, const size_t *n_floats, pf_plan &p, std::vector<float> &host);

}  // namespace pf
