// The bg training step as its three translation units share it (not part of the ABI): train_layout.cpp describes the net and lays out
// the workspace, train_schedule.cpp writes the step as a flat list of TSteps (both host code only: no HIP call, no device property),
// train_plan.hip owns the streams and events and enqueues the list.
#pragma once
#include <array>
#include <map>
#include <vector>

#include "hardnet_plan.h"
#include "train_kernels.h"

namespace pf {

// the process-wide switches of the training step (defined in train_plan.hip; pf_set_option: plan_create.hip)
extern int g_opt_up_two_pass, g_opt_train_table_batch, g_opt_train_kacc, g_opt_train_s4, g_opt_train_side;

// kSideStreams side streams, layer n on stream n % kSideStreams; kDySlots conv-output-gradient buffers decouple the two sides:
// the caller's stream may run kDySlots layers ahead of the weight gradients
constexpr int kSideStreams = 1, kDySlots = 4;
static_assert(kDySlots % kSideStreams == 0, "a dy slot belongs to one side stream");

// ---- train_layout.cpp
// The net as a training plan holds it on the host, with the switches that are fixed when the plan is created
struct TrainNet {
    NetTable net;
    std::vector<size_t> w_off, aux_off;   // per op (floats into theta); aux = gamma (BN) or bias
    std::vector<int> bn;                  // per op: 1 = conv + BN (+ ReLU), 0 = plain conv with bias
    size_t n_params = 0;
    int fwd_s4 = 0;                       // option "train_forward_s4": forward convolutions on conv_s4 (train_s4.hip)
    int side = 0;                         // option "train_side_stream": the weight gradients on the plan's side streams
};
// the op table of the blob, the parameter layout and the two options as they are now
int train_net_init(const void *blob, size_t bytes, int in_ch, int n_cls, TrainNet &n);

// Who writes a tensor's gradient first?  The backward pass visits the ops in reverse; every consumer of a tensor adds its
// contribution to the tensor's gradient.  The first visitor of a channel range STORES instead (no cleared arena needed: the
// arena is as large as all activations, 0.2 ms of fill per step at batch 8 of 800x800); a range that is only partly fresh keeps
// the add and has its fresh channels cleared beforehand, as are channels no consumer ever writes (their producer reads them).
struct GradFirst {
    std::vector<std::array<uint8_t, kConvMaxSrc>> store;     // per op, per input range (conv / stem) or [0] (pool, upsample, head)
    std::vector<std::array<int, 3>> clear;               // (tensor, first channel, channels)
};
GradFirst grad_first_writers(const TrainNet &n, const std::vector<Dims> &d);

struct TLayout {
    std::vector<size_t> act, grad;     // per tensor (bytes); act[input] = the dense one-hot/depth tensor
    std::vector<size_t> ypre, stat;    // per op: pre-BN conv output, {mean[cout], invstd[cout]}
    // per conv op: stride 1 on a width that is not a multiple of 4 - its output keeps rows padded to 4 (ypre, dy), and ONE
    // backward-data conv covers all its input ranges
    std::vector<uint8_t> odd;
    std::vector<size_t> xpad;          // per odd op: its gathered, row-padded input, kept from the forward pass for the weight gradient
    size_t dy = 0, wpart = 0, dfull = 0, cepart = 0, bnpart = 0, out3 = 0, total = 0;
    size_t pad_in = 0, pad_out = 0;    // odd-width convs: gathered input / result with the row pitch rounded up to 4
    size_t dy_more[kDySlots] = {}, wpart_more[kSideStreams] = {};   // side streams: further dy slots, per stream the partial sums
    size_t up_tmp = 0;                 // scratch of the two-pass bilinear transpose
    size_t tune_grad = 0;              // autotune: the measuring pass's parameter gradients (discarded)
    // every tiled weight packing of the step (forward convs in op order, then the backward-data convs of every op and input
    // range in op order): packed by ONE batch of launches at the start of the step into wpk_arena
    std::vector<PackJob> jobs;
    std::vector<int> fwd_job;                  // per op: its forward job, or -1
    std::vector<std::vector<int>> bwd_job;     // per op, per input range: its backward-data job, or -1 (the network input needs none)
    std::vector<int> bwd_all_job;              // per op of an odd-width level: ONE backward-data conv over all input ranges, or -1
    size_t wpk_arena = 0;
    // forward pass on the packed-pair kernels (train_s4.hip): per tensor its shadow, per op its device-side weight packing
    std::vector<size_t> s4act;
    std::vector<int> s4_job;
    std::vector<S4WJob> s4jobs;
    size_t s4w_arena = 0;
};
// one region of the workspace as t_layout hands it out (pf_debug_train_plan; include/pfhip.h lists the kinds)
enum TRegionKind { R_ACT, R_GRAD, R_YPRE, R_STAT, R_XPAD, R_WPK, R_S4ACT, R_S4W, R_TUNE_GRAD, R_DY, R_WPART, R_PAD_IN, R_PAD_OUT, R_DFULL,
                   R_UP_TMP, R_CEPART, R_BNPART, R_OUT3, R_TOTAL };
struct TRegion { int kind, index; size_t off, bytes; };
// autotune: room for the measuring pass's gradients (pf_train_autotune).  regions (nullable): every region in the order it was handed out
TLayout t_layout(const TrainNet &n, bool autotune, int B, const std::vector<Dims> &d, int out_h, int out_w, std::vector<TRegion> *regions = nullptr);

// ---- train_schedule.cpp
// the arguments of one pf_train_forward_backward
struct TCall {
    float *theta, *grad;
    int accumulate_grads;
    const void *seg; int seg_is_i64; const float *depth; const uint8_t *depth_mask; float depth_mean, depth_std; int T;
    const float *x_dense; int B, H, W;
    const void *labels; int labels_i64, out_h, out_w, ignore_index;
    float loss_scale, bn_momentum, bn_eps; int update_running_stats;
    double *out3; void *ws; size_t ws_bytes; hipStream_t s;
};

// ---- One step of the schedule: a kernel (its arguments in the member of `u` named after it) or a stream operation of the side
//      streams (fork = record ev_dy[slot] on the caller's stream + wait on the side stream; wg_done = record ev_wg[slot] on the side
//      stream; wait_wg = the caller's stream waits for it before the slot is overwritten)
enum TStepKind : uint8_t {
    T_COPY, T_ONEHOT, T_PACK_TILED, T_PACK_S4, T_ZERO_CHANNELS, T_ZERO_FILL,
    T_PAD_GATHER, T_CONV_DMA, T_CONV_DMA_MEASURE, T_CONV_S4, T_UNPAD, T_UNPAD_MULTI, T_BN_FWD, T_S4_ACT, T_POOL, T_UPSAMPLE, T_CE,
    T_UPSAMPLE_BWD, T_POOL_BWD, T_BN_BWD, T_BIAS_BWD, T_ZERO_STUFF, T_WGRAD, T_WAIT_WG, T_FORK, T_WG_DONE };
struct TCopyArgs { void *dst; const void *src; size_t bytes; };       // copy; zero fill (src unused)
struct TOneHotArgs { const void *seg; int seg_i64; const float *depth; const uint8_t *mask; float mean, stdv; int T, n_cls, H, W; float *x; };
struct TPackArgs { const float *theta; float *arena; const void *jobs; int n; };   // PackJob / S4WJob list
struct TZeroChArgs { float *t; int ctotal, c0, n; long long hw; };
struct TGatherArgs { ConvArgs a; int Wp; float *dst; };               // the ranges of a -> dst with rows of Wp pixels
// conv_dma: wm x nt (measure: chosen at enqueue); conv_s4: the instantiation s4
struct TConvArgs { ConvArgs a; int ks, stride, wm, nt; S4Shape s4; };
struct TUnpadArgs { const float *src; int C, H, W, Wp; float *dst; int ctotal, choff, accum; };
struct TUnpadMultiArgs { const float *src; int C, H, W, Wp, n; float *dst[kConvMaxSrc]; int ctotal[kConvMaxSrc], choff[kConvMaxSrc], ch[kConvMaxSrc], overwrite[kConvMaxSrc]; };
struct TBnFwdArgs {
    const float *y; int C, H, W; float eps, momentum; const float *gamma, *beta; float *rmean, *rvar, *mean, *invstd; double *part;
    float *dst; int dst_ctotal, dst_choff, relu, y_pitch;
};
struct TS4ActArgs { const float *src; int ctotal, c0, c1, fill_lo, fill_up, H, W, Wp; void *dst; };
// pool, upsample, zero-stuff: [planes][hin][win] -> [planes][hout][wout]; pool backward: dst (+)= from src, overwrite
struct TPlainArgs { const float *src; float *dst; int planes, hin, win, hout, wout, overwrite; };
struct TCeArgs { const float *logits; int C, hi, wi; const void *labels; int lab_i64, ho, wo, ignore; float *dfull; double *part, *out3; };
struct TUpBwdArgs { const float *gout; int planes, hi, wi, ho, wo; const double *count; float scale; int accumulate; float *gin, *tmp; };
struct TBnBwdArgs {      // (bias backward: g .. choff, C, H, W, dgamma = dbias, part, dy, dy_pitch)
    const float *g; int t_ctotal, choff; const float *y, *mean, *invstd, *gamma, *beta; int C, H, W, relu; float *dgamma, *dbeta;
    double *part; float *dy; int dy_pitch, y_pitch;
};
// a: the forward conv; tag: profile tag of its launches (set when profiling)
struct TWgradArgs { ConvArgs a; int ks, stride; const float *dy; float *partial, *dw; char tag[64]; };
struct TStep {
    TStepKind kind;
    uint8_t stats;       // bit k: the step counts in pf_train_path_stats slot k
    int side, slot;      // side stream of the step (-1: the caller's stream); the dy slot of fork / wait_wg / wg_done
    union {
        TCopyArgs copy; TOneHotArgs onehot; TPackArgs pack; TZeroChArgs zch; TGatherArgs gather; TConvArgs conv; TUnpadArgs unpad;
        TUnpadMultiArgs unpadm; TBnFwdArgs bnf; TS4ActArgs s4act; TPlainArgs plain; TCeArgs ce; TUpBwdArgs upb; TBnBwdArgs bnb; TWgradArgs wg;
    } u;
};

// pf_train_autotune: (ks, stride, Cin, Cout, Hin, Win, B, accum) -> the measured (wm, nt)
typedef std::map<std::array<int, 8>, std::pair<int, int>> TunedMap;
inline std::array<int, 8> tune_key(const ConvArgs &c, int ks, int stride, int B) { return {ks, stride, c.Cin, c.Cout, c.Hin, c.Win, B, c.accum}; }

// The whole step (input, weight packings, gradient clears, forward, loss, backward) into `steps`, every argument resolved into
// the call's theta, gradient and workspace.  Kernel choices are made here, through predicates: a geometry without a kernel
// fails before anything is enqueued.  zero_page: the plan's 1024 zeros; tuned (nullable): what pf_train_autotune has measured;
// measuring: the autotune pass - a conv_dma geometry not in `tuned` is measured at enqueue time (T_CONV_DMA_MEASURE)
int build_train_schedule(const TrainNet &n, const TCall &k, const std::vector<Dims> &d, const TLayout &L, const GradFirst &gfirst,
                         const float *zero_page, const TunedMap *tuned, bool measuring, std::vector<TStep> &steps);

}  // namespace pf
