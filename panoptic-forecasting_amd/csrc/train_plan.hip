// bg training step (scope row f4): forward in training mode + loss + backward over the op table, and the optimiser step.
//
// Replaces, for task `bg`, what the reference's training loop does per batch (training/train.py:185-222):
//     loss_dict = model.loss(inputs, labels)      models/bg/bg_model.py:73-89  (train-mode BatchNorm, F.interpolate, CrossEntropyLoss)
//     loss.backward()                             autograd through hardnet.py:353-387
//     clip_grad_value_ / clip_grad_norm_ ; opt.step()  (SGD, momentum, weight decay: train.py:130-138)
// Parameters live in ONE flat fp32 arena `theta` (layout below; the Python side maps the reference's state_dict keys onto
// it), gradients in an arena of the same layout — so the data-parallel exchange is a single all-reduce of ~16.5 MB over
// RCCL between pf_train_forward_backward and pf_sgd_step (the reference wraps the model in DDP, train.py:96-103).
//
// theta layout: for every conv op of the table, in table order:  W[cout][cin][k][k],  then
//     with BatchNorm:  gamma[cout], beta[cout], running_mean[cout], running_var[cout]      (ConvLayer, hardnet.py:16-25)
//     without       :  bias[cout]                                                          (finalConv, hardnet.py:325-327)
//
// Convolutions run on the fp32 matrix cores: forward and backward-data through the LDS-DMA kernels of the inference path
// (conv_dma.hip; widths that are not a multiple of 4 on copies with padded rows) with the weights re-packed on the device
// every step (forward order, or transposed + flipped per input range; stride-2 backward-data = stride-1 conv over the
// zero-stuffed gradient; a tensor's gradient accumulates over its consumers in the store), backward-weight through the
// LDS-tiled wgrad kernels of train_kernels.hip.
//
// A step = build_train_schedule (host code only: the whole step as a flat list of TSteps, each naming exactly one kernel or
// stream operation with all of its arguments; every kernel and shape is chosen there through predicates, so a geometry
// without a kernel fails before anything is enqueued) + the enqueue loop of train_pass, a switch with one call per step.
#include <algorithm>
#include <array>
#include <cstring>
#include <map>
#include <vector>

#include "hardnet_plan.h"
#include "pf_prof.h"
#include "train_kernels.h"

using namespace pf;

#ifndef PF_TRAIN_SIDE_STREAMS
#define PF_TRAIN_SIDE_STREAMS 1
#endif
#ifndef PF_TRAIN_DY_SLOTS
#define PF_TRAIN_DY_SLOTS 4
#endif
static_assert(PF_TRAIN_DY_SLOTS % PF_TRAIN_SIDE_STREAMS == 0, "a dy slot belongs to one side stream");

struct pf_train {
    NetTable net;
    std::vector<size_t> w_off, aux_off;   // per op (floats into theta); aux = gamma (BN) or bias
    std::vector<int> bn;                  // per op: 1 = conv + BN (+ ReLU), 0 = plain conv with bias
    size_t n_params = 0;
    float *dev_zero = nullptr;            // 1024 zeros (the zero bias and zero page of the conv launches)
    // the weight gradients are leaves of the backward pass: they run on this plan's own lower-priority stream, forked from and
    // joined to the caller's stream inside every pf_train_forward_backward (so a stream capture of the call stays one graph).
    // Option "train_side_stream" (read when the plan is created; 0 = everything on the caller's stream)
    // kSideStreams of them, layer n on stream n % kSideStreams; kDySlots conv-output-gradient buffers decouple the two sides:
    // the caller's stream may run kDySlots layers ahead of the weight gradients
    static constexpr int kSideStreams = PF_TRAIN_SIDE_STREAMS, kDySlots = PF_TRAIN_DY_SLOTS;
    hipStream_t side = nullptr;             // == sides[0]; non-null <=> the side streams are in use
    hipStream_t sides[kSideStreams] = {};
    hipEvent_t ev_dy[kDySlots] = {}, ev_wg[kDySlots] = {}, ev_join[kSideStreams] = {};
    // pf_train_autotune: the workgroup shape (pixel waves x cout tiles) of every forward / backward-data convolution is MEASURED
    // the first time its geometry is seen outside a stream capture (every candidate of conv_dma's shape list, 3 launches each,
    // hipEvents) instead of taken from the inference path's cost model, which was calibrated on 1024x2048 batches.  Off by default:
    // the choice (and with it the summation order of K-split shapes) then depends on timing, i.e. may differ from run to run.
    int autotune = 0;
    int fwd_s4 = 0;                       // option "train_forward_s4" when the plan was created: forward convolutions on conv_s4 (train_s4.hip)
    mutable std::map<std::array<int, 8>, std::pair<int, int>> tuned;   // (ks, stride, Cin, Cout, Hin, Win, B, accum) -> (wm, nt)
    mutable hipEvent_t tune_ev[2] = {nullptr, nullptr};
    // pf_train_path_stats: which code paths the LAST pf_train_forward_backward took, counted from its schedule (tests assert that
    // a timed configuration really ran the table's shapes and the padded odd-width forms)
    mutable int stats[8] = {};
    mutable std::vector<std::array<int, 5>> measured_configs;
};

namespace pf {   // the process-wide switches of the training step (pf_set_option: plan_create.hip)
int g_opt_up_two_pass = 1;         // upsample_bwd_two_pass: the bilinear transposes of large planes as rows-then-columns passes (train_kernels.hip)
int g_opt_train_table_batch = 0;   // train_table_batch: batch size the rows of train_tuned.inc are looked up with (0 = the call's own)
int g_opt_train_kacc = 1;          // train_blocked_sum: per-round partial sums in the 3x3 convolutions of a training step (conv_dma.hip: KACC)
int g_opt_train_s4 = 0;            // train_forward_s4: the forward convolutions of a training step on conv_s4 with blocked sums (train_s4.hip); opt-in
int g_opt_train_side = 1;          // train_side_stream: weight gradients on the training plan's own stream
}

namespace {

// measured shapes of the training step's convolutions for the configurations tools/tune_train.py was run on (the reference's
// configs/bg/bg_train.yaml: batch 8 of 800x800 crops): {ks, stride, Cin, Cout, Hin, Win, B, accum, wm, nt}.  Consulted when option
// "use_tuned_table" is on (default) and the plan does not measure for itself; other geometries take the cost model's shape
struct TrainTuned {
    int key[8], wm, nt;
};
const TrainTuned kTrainTuned[] = {
#include "train_tuned.inc"
    {{0, 0, 0, 0, 0, 0, 0, 0}, 0, 0}};

// Who writes a tensor's gradient first?  The backward pass visits the ops in reverse; every consumer of a tensor adds its
// contribution to the tensor's gradient.  The first visitor of a channel range STORES instead (no cleared arena needed: the
// arena is as large as all activations, 0.2 ms of fill per step at batch 8 of 800x800); a range that is only partly fresh keeps
// the add and has its fresh channels cleared beforehand, as are channels no consumer ever writes (their producer reads them).
struct GradFirst {
    std::vector<std::array<uint8_t, kConvMaxSrc>> store;     // per op, per input range (conv / stem) or [0] (pool, upsample, head)
    std::vector<std::array<int, 3>> clear;               // (tensor, first channel, channels)
};
GradFirst grad_first_writers(const pf_train *p, const std::vector<Dims> &d) {
    GradFirst g;
    g.store.assign(p->net.ops.size(), std::array<uint8_t, kConvMaxSrc>{});
    const uint32_t input = p->net.ops[0].src[0].tensor;
    std::vector<std::vector<uint8_t>> touched(p->net.tensors.size());
    for (size_t t = 0; t < p->net.tensors.size(); ++t) touched[t].assign(p->net.tensors[t].channels, 0);
    auto add_clear = [&](uint32_t t, const std::vector<uint8_t> &want) {       // runs of channels
        for (size_t c = 0; c < want.size();) {
            if (!want[c]) { ++c; continue; }
            size_t e = c;
            while (e < want.size() && want[e]) ++e;
            g.clear.push_back({(int)t, (int)c, (int)(e - c)});
            c = e;
        }
    };
    for (size_t ii = p->net.ops.size(); ii-- > 0;) {
        const BlobOp &o = p->net.ops[ii];
        const uint32_t nj = (o.kind == OP_STEM || o.kind == OP_CONV) ? o.n_src : 1;
        for (uint32_t j = 0; j < nj; ++j) {
            const uint32_t t = o.src[j].tensor;
            if (t == input) continue;
            const bool whole = !(o.kind == OP_STEM || o.kind == OP_CONV);      // pool / upsample / head write the whole tensor
            const uint32_t c0 = whole ? 0 : o.src[j].choff, n = whole ? p->net.tensors[t].channels : o.src[j].ch;
            uint32_t fresh = 0;
            for (uint32_t c = c0; c < c0 + n; ++c) fresh += !touched[t][c];
            if (fresh == n) {
                g.store[ii][j] = 1;
            } else if (fresh) {
                std::vector<uint8_t> want(p->net.tensors[t].channels, 0);
                for (uint32_t c = c0; c < c0 + n; ++c) want[c] = !touched[t][c];
                add_clear(t, want);
            }
            for (uint32_t c = c0; c < c0 + n; ++c) touched[t][c] = 1;
        }
    }
    for (size_t t = 0; t < p->net.tensors.size(); ++t) {
        if (t == input || !d[t].h) continue;
        std::vector<uint8_t> want(p->net.tensors[t].channels, 0);
        bool any = false;
        for (size_t c = 0; c < want.size(); ++c) any |= (want[c] = !touched[t][c]) != 0;
        if (any) add_clear((uint32_t)t, want);
    }
    return g;
}

struct TLayout {
    std::vector<size_t> act, grad;     // per tensor (bytes); act[input] = the dense one-hot/depth tensor
    std::vector<size_t> ypre, stat;    // per op: pre-BN conv output, {mean[cout], invstd[cout]}
    // per conv op: stride 1 on a width that is not a multiple of 4 - its output keeps rows padded to 4 (ypre, dy), and ONE
    // backward-data conv covers all its input ranges
    std::vector<uint8_t> odd;
    std::vector<size_t> xpad;          // per odd op: its gathered, row-padded input, kept from the forward pass for the weight gradient
    size_t dy = 0, wpart = 0, dfull = 0, cepart = 0, bnpart = 0, out3 = 0, total = 0;
    size_t pad_in = 0, pad_out = 0;    // odd-width convs: gathered input / result with the row pitch rounded up to 4
    size_t dy_more[pf_train::kDySlots] = {}, wpart_more[pf_train::kSideStreams] = {};   // side streams: further dy slots, per stream the partial sums
    size_t up_tmp = 0;                 // scratch of the two-pass bilinear transpose
    size_t tune_grad = 0;              // autotune: the measuring pass's parameter gradients (discarded)
    size_t grad_begin = 0, grad_end = 0;
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

// may op i's forward convolution run on conv_s4?  conv + BatchNorm, 3x3 / 1x1, stride 1, every input range at an even channel of a
// tensor some op produced (the network input stays dense fp32: the stem reads it)
bool s4_fwd_ok(const pf_train *p, size_t i) {
    const BlobOp &o = p->net.ops[i];
    if (!p->fwd_s4 || o.kind != OP_CONV || !p->bn[i] || o.stride != 1 || (o.k != 1 && o.k != 3) || o.n_src > (uint32_t)kConvMaxSrc) return false;
    const uint32_t input = p->net.ops[0].src[0].tensor;
    for (uint32_t j = 0; j < o.n_src; ++j)
        if ((o.src[j].choff & 1) || o.src[j].tensor == input) return false;
    return true;
}

TLayout t_layout(const pf_train *p, int B, const std::vector<Dims> &d, int out_h, int out_w) {
    TLayout L;
    const size_t nt = p->net.tensors.size();
    L.act.assign(nt, (size_t)-1);
    L.grad.assign(nt, (size_t)-1);
    L.ypre.assign(p->net.ops.size(), (size_t)-1);
    L.stat.assign(p->net.ops.size(), (size_t)-1);
    L.xpad.assign(p->net.ops.size(), (size_t)-1);
    size_t cur = 0;
    auto take = [&](size_t bytes) {
        const size_t o = cur;
        cur += align_up(bytes, 256);
        return o;
    };
    auto tbytes = [&](size_t t) { return (size_t)B * p->net.tensors[t].channels * d[t].h * d[t].w * sizeof(float); };
    for (size_t t = 0; t < nt; ++t)
        if (d[t].h) L.act[t] = take(tbytes(t));
    L.grad_begin = cur;
    const uint32_t input = p->net.ops[0].src[0].tensor;
    for (size_t t = 0; t < nt; ++t)
        if (d[t].h && t != input) L.grad[t] = take(tbytes(t));
    L.grad_end = cur;
    L.odd.assign(p->net.ops.size(), 0);
    size_t max_dy = 0, max_wpart = 0, max_c = 16, max_pin = 256, max_pout = 256;
    for (size_t i = 0; i < p->net.ops.size(); ++i) {
        const BlobOp &o = p->net.ops[i];
        if (o.kind != OP_STEM && o.kind != OP_CONV) continue;
        const Dims in = d[o.src[0].tensor], out = d[o.dst];
        L.odd[i] = (in.w & 3) && o.stride == 1;
        // the conv output (y, dy) in padded rows on an odd level
        const size_t ybytes = (size_t)B * o.cout * out.h * (L.odd[i] ? (out.w + 3) / 4 * 4 : out.w) * sizeof(float);
        if (p->bn[i]) {
            L.ypre[i] = take(ybytes);
            L.stat[i] = take(2 * (size_t)o.cout * sizeof(float));
        }
        // dy scratch: the conv-output gradient, and (stride 2) its zero-stuffed copy at the input resolution
        size_t need = ybytes;
        if (o.stride == 2) need += align_up((size_t)B * o.cout * in.h * in.w * sizeof(float), 256);
        max_dy = need > max_dy ? need : max_dy;
        if (L.odd[i]) L.xpad[i] = take((size_t)B * o.cin * in.h * ((in.w + 3) / 4 * 4) * sizeof(float));
        if (in.w & 3) {     // padded copies (forward: cin -> cout at the output size; backward-data: cout -> cin at the input size)
            const size_t wp_in = (size_t)(in.w + 3) / 4 * 4, cmax = o.cin > o.cout ? o.cin : o.cout;
            const size_t bytes = (size_t)B * cmax * in.h * wp_in * sizeof(float);
            max_pin = bytes > max_pin ? bytes : max_pin;
            max_pout = bytes > max_pout ? bytes : max_pout;
        }
        const int wpi = o.stride == 1 ? (in.w + 3) / 4 * 4 : in.w, wpo = o.stride == 1 ? (out.w + 3) / 4 * 4 : out.w;   // (padded copies for odd widths)
        const size_t wp = wgrad_partial_floats((int)o.cout, (int)o.cin, (int)o.k, B, out.h, wpi, wpo);
        max_wpart = wp > max_wpart ? wp : max_wpart;
        max_c = o.cout > max_c ? o.cout : max_c;
    }
    // the step's packing jobs (the padded copies of odd-width levels read ONE gathered range)
    {
        L.fwd_job.assign(p->net.ops.size(), -1);
        L.bwd_job.assign(p->net.ops.size(), std::vector<int>());
        L.bwd_all_job.assign(p->net.ops.size(), -1);
        size_t arena = 0;
        auto add = [&](size_t w_off, int cin_f, int cout_f, int ks, int stride, const int *chs, int ns, int tflip, int c0, int ch) {
            PackJob q;
            pack_job_fill(q, w_off, cin_f, cout_f, ks, stride, chs, ns, tflip, c0, ch, arena);
            arena += align_up((size_t)q.total, 64);
            L.jobs.push_back(q);
            return (int)L.jobs.size() - 1;
        };
        for (size_t i = 0; i < p->net.ops.size(); ++i) {
            const BlobOp &o = p->net.ops[i];
            if (o.kind != OP_STEM && o.kind != OP_CONV) continue;
            const Dims in = d[o.src[0].tensor];
            int src_ch[kConvMaxSrc];
            for (uint32_t j = 0; j < o.n_src; ++j) src_ch[j] = (int)o.src[j].ch;
            const int one = (int)o.cin;
            const bool aligned = (in.w & 3) == 0;
            L.fwd_job[i] = add(p->w_off[i], (int)o.cin, (int)o.cout, (int)o.k, (int)o.stride, aligned ? src_ch : &one, aligned ? (int)o.n_src : 1, 0, 0, 0);
        }
        for (size_t i = 0; i < p->net.ops.size(); ++i) {
            const BlobOp &o = p->net.ops[i];
            if (o.kind != OP_STEM && o.kind != OP_CONV) continue;
            L.bwd_job[i].assign(o.n_src, -1);
            const int dy_ch = (int)o.cout;
            if (L.odd[i]) {
                L.bwd_all_job[i] = add(p->w_off[i], (int)o.cin, (int)o.cout, (int)o.k, 1, &dy_ch, 1, 1, 0, (int)o.cin);
                continue;
            }
            const KOrder ko = order_plain(o.src, (int)o.n_src);
            for (int j = 0; j < ko.n; ++j)
                if (ko.r[j].tensor != input) L.bwd_job[i][j] = add(p->w_off[i], (int)o.cin, (int)o.cout, (int)o.k, 1, &dy_ch, 1, 1, ko.r[j].cstart, ko.r[j].ch);
        }
        L.wpk_arena = take(arena * sizeof(float) + 256);
    }
    // the forward convolutions that run on the packed-pair kernels: their device-side weight packings, and the shadows of the tensors they read
    {
        L.s4act.assign(nt, (size_t)-1);
        L.s4_job.assign(p->net.ops.size(), -1);
        std::vector<char> need(nt, 0);
        size_t arena = 0;
        for (size_t i = 0; i < p->net.ops.size(); ++i) {
            if (!s4_fwd_ok(p, i)) continue;
            const BlobOp &o = p->net.ops[i];
            for (uint32_t j = 0; j < o.n_src; ++j) need[o.src[j].tensor] = 1;
            S4WJob jb;
            const size_t fl = s4_wjob_init(jb, p->w_off[i], (int)o.cin, (int)o.cout, (int)o.k, order_plain(o.src, (int)o.n_src), o.k == 1 && o.n_src == 2);
            jb.out_off = (unsigned)arena;
            arena += align_up(fl, 64);
            L.s4_job[i] = (int)L.s4jobs.size();
            L.s4jobs.push_back(jb);
        }
        for (size_t t = 0; t < nt; ++t)
            if (need[t] && d[t].h) L.s4act[t] = take((size_t)B * 2 * ((p->net.tensors[t].channels + 3) / 4) * d[t].h * ((d[t].w + 3) / 4 * 4) * 8);
        L.s4w_arena = take(arena * sizeof(float) + 256);
    }
    if (p->autotune) L.tune_grad = take(p->n_params * sizeof(float));
    L.dy = take(max_dy + 256);
    if (p->side)
        for (int k = 1; k < pf_train::kDySlots; ++k) L.dy_more[k] = take(max_dy + 256);
    L.wpart = take(max_wpart * sizeof(float));
    if (p->side)
        for (int k = 1; k < pf_train::kSideStreams; ++k) L.wpart_more[k] = take(max_wpart * sizeof(float));
    L.pad_in = take(max_pin);
    L.pad_out = take(max_pout);
    L.dfull = take((size_t)B * p->net.hdr.n_cls * out_h * out_w * sizeof(float));
    {
        size_t mx = 0;
        for (size_t i = 0; i < p->net.ops.size(); ++i) {
            const BlobOp &o = p->net.ops[i];
            const Dims in = d[o.src[0].tensor];
            size_t n = 0;
            if (o.kind == OP_HEAD) n = upsample_bwd_tmp_floats(B * (int)o.cin, in.h, in.w, out_h, out_w);
            else if (o.kind == OP_UPSAMPLE) n = upsample_bwd_tmp_floats(B * (int)o.cin, in.h, in.w, d[o.dst].h, d[o.dst].w);
            mx = n > mx ? n : mx;
        }
        L.up_tmp = take(mx * sizeof(float) + 256);
    }
    L.cepart = take(ce_partial_doubles(B, out_h, out_w) * sizeof(double));
    L.bnpart = take(bn_partial_doubles((int)max_c) * sizeof(double));
    L.out3 = take(4 * sizeof(double));
    L.total = cur;
    return L;
}

}  // namespace

extern "C" int pf_train_create(const void *blob, size_t bytes, int in_ch, int n_cls, pf_train **out) {
    if (!blob || !out) return fail(PF_EINVAL, "pf_train_create: null argument");
    pf_train *p = new pf_train();
    if (int rc = parse_net_table(blob, bytes, in_ch, n_cls, p->net)) {
        delete p;
        return rc;
    }
    const size_t n_ops = p->net.ops.size();
    p->w_off.assign(n_ops, 0);
    p->aux_off.assign(n_ops, 0);
    p->bn.assign(n_ops, 0);
    size_t cur = 0;
    for (size_t i = 0; i < n_ops; ++i) {
        const BlobOp &o = p->net.ops[i];
        if (o.kind != OP_STEM && o.kind != OP_CONV) continue;
        uint32_t cin = 0;
        for (uint32_t j = 0; j < o.n_src; ++j) cin += o.src[j].ch;
        if (cin != o.cin || !((o.k == 3 && (o.stride == 1 || o.stride == 2)) || (o.k == 1 && o.stride == 1))) {
            delete p;
            return fail(PF_EUNSUPPORTED, "op %zu: training supports 3x3 (stride 1/2) and 1x1 convs", i);
        }
        // packing.py writes pad[0] = 1 + has_bn; blobs without the field: ConvLayer (conv + BN + ReLU) <=> relu flag
        p->bn[i] = o.pad[0] ? (int)o.pad[0] - 1 : (int)(o.relu != 0);
        p->w_off[i] = cur;
        cur += (size_t)o.cout * o.cin * o.k * o.k;
        p->aux_off[i] = cur;
        cur += (size_t)o.cout * (p->bn[i] ? 4 : 1);
    }
    p->n_params = cur;
    if (hipMalloc((void **)&p->dev_zero, 1024 * sizeof(float)) != hipSuccess || hipMemset(p->dev_zero, 0, 1024 * sizeof(float)) != hipSuccess) {
        delete p;
        return fail(PF_EHIP, "pf_train_create: device allocation failed");
    }
    p->fwd_s4 = g_opt_train_s4;
    if (g_opt_train_side) {
        int lo = 0, hi = 0;
        bool ok = hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess;
        for (int k = 0; ok && k < pf_train::kSideStreams; ++k) ok = hipStreamCreateWithPriority(&p->sides[k], hipStreamNonBlocking, lo) == hipSuccess;
        p->side = p->sides[0];
        for (int k = 0; ok && k < pf_train::kDySlots; ++k)
            ok = hipEventCreateWithFlags(&p->ev_dy[k], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&p->ev_wg[k], hipEventDisableTiming) == hipSuccess;
        for (int k = 0; ok && k < pf_train::kSideStreams; ++k) ok = hipEventCreateWithFlags(&p->ev_join[k], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            pf_train_destroy(p);
            return fail(PF_EHIP, "pf_train_create: could not create the weight-gradient stream");
        }
    }
    *out = p;
    return PF_OK;
}

extern "C" void pf_train_destroy(pf_train *p) {
    if (!p) return;
    for (int k = 0; k < pf_train::kDySlots; ++k) {
        if (p->ev_dy[k]) (void)hipEventDestroy(p->ev_dy[k]);
        if (p->ev_wg[k]) (void)hipEventDestroy(p->ev_wg[k]);
    }
    for (hipEvent_t e : p->tune_ev)
        if (e) (void)hipEventDestroy(e);
    for (int k = 0; k < pf_train::kSideStreams; ++k) {
        if (p->ev_join[k]) (void)hipEventDestroy(p->ev_join[k]);
        if (p->sides[k]) (void)hipStreamDestroy(p->sides[k]);
    }
    if (p->dev_zero) (void)hipFree(p->dev_zero);
    delete p;
}

extern "C" int pf_train_autotune(pf_train *p, int enable) {
    if (!p) return fail(PF_EINVAL, "pf_train_autotune: null plan");
    p->autotune = enable != 0;      // (changes pf_train_workspace: the measuring pass has its own parameter-gradient buffer)
    if (!enable) {
        p->tuned.clear();
        p->measured_configs.clear();
    }
    return PF_OK;
}

extern "C" int pf_train_tuned_shapes(const pf_train *p, int *rows, int cap_rows, int *n_rows) {
    if (!p || !n_rows || (cap_rows > 0 && !rows)) return fail(PF_EINVAL, "pf_train_tuned_shapes: null argument");
    *n_rows = (int)p->tuned.size();
    int i = 0;
    for (const auto &kv : p->tuned) {
        if (i >= cap_rows) break;
        for (int k = 0; k < 8; ++k) rows[i * 10 + k] = kv.first[k];
        rows[i * 10 + 8] = kv.second.first;
        rows[i * 10 + 9] = kv.second.second;
        ++i;
    }
    return PF_OK;
}

extern "C" int pf_train_path_stats(const pf_train *p, int *stats, int cap, int *n) {
    if (!p || !n || (cap > 0 && !stats)) return fail(PF_EINVAL, "pf_train_path_stats: null argument");
    *n = 8;
    for (int k = 0; k < 8 && k < cap; ++k) stats[k] = p->stats[k];
    return PF_OK;
}

extern "C" int pf_train_param_count(const pf_train *p, size_t *n_floats) {
    if (!p || !n_floats) return fail(PF_EINVAL, "pf_train_param_count: null");
    *n_floats = p->n_params;
    return PF_OK;
}

extern "C" int pf_train_param_layout(const pf_train *p, int op_index, size_t *w_off, size_t *aux_off, int *has_bn) {
    if (!p || op_index < 0 || (size_t)op_index >= p->net.ops.size() || !w_off || !aux_off || !has_bn) return fail(PF_EINVAL, "pf_train_param_layout: bad argument");
    const BlobOp &o = p->net.ops[op_index];
    if (o.kind != OP_STEM && o.kind != OP_CONV) return fail(PF_EINVAL, "op %d is not a convolution", op_index);
    *w_off = p->w_off[op_index];
    *aux_off = p->aux_off[op_index];
    *has_bn = p->bn[op_index];
    return PF_OK;
}

extern "C" int pf_train_workspace(const pf_train *p, int B, int H, int W, int out_h, int out_w, size_t *bytes) {
    if (!p || !bytes || B <= 0 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0) return fail(PF_EINVAL, "pf_train_workspace: bad argument");
    std::vector<Dims> d;
    int rc = propagate_dims(p->net, H, W, d);
    if (rc) return rc;
    *bytes = t_layout(p, B, d, out_h, out_w).total;
    return PF_OK;
}

extern "C" int pf_train_tensor_view(const pf_train *p, const char *name, int want_grad, int B, int H, int W, int out_h, int out_w,
                                    size_t *ws_offset, int *channels, int *h, int *w) {
    if (!p || !name || !ws_offset || !channels || !h || !w) return fail(PF_EINVAL, "pf_train_tensor_view: null");
    std::vector<Dims> d;
    int rc = propagate_dims(p->net, H, W, d);
    if (rc) return rc;
    const TLayout L = t_layout(p, B, d, out_h, out_w);
    for (size_t t = 0; t < p->net.tensors.size(); ++t)
        if (strncmp(p->net.tensors[t].name, name, sizeof(p->net.tensors[t].name)) == 0) {
            const size_t off = want_grad ? L.grad[t] : L.act[t];
            if (off == (size_t)-1) return fail(PF_EINVAL, "tensor '%s' has no %s buffer", name, want_grad ? "gradient" : "activation");
            *ws_offset = off; *channels = (int)p->net.tensors[t].channels; *h = d[t].h; *w = d[t].w;
            return PF_OK;
        }
    return fail(PF_EINVAL, "no tensor named '%s'", name);
}

namespace {

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

// ---- One step of the schedule: a kernel (its arguments in the member of `u` named after it, convolutions in `a`) or a stream
//      operation of the side streams (fork = record ev_dy[slot] on the caller's stream + wait on the side stream; wg_done = record
//      ev_wg[slot] on the side stream; wait_wg = the caller's stream waits for it before the slot is overwritten)
enum TStepKind : uint8_t {
    T_COPY, T_ONEHOT, T_PACK_TILED, T_PACK_S4, T_ZERO_CHANNELS, T_ZERO_FILL,
    T_PAD_GATHER, T_CONV_DMA, T_CONV_DMA_MEASURE, T_CONV_S4, T_UNPAD, T_UNPAD_MULTI, T_BN_FWD, T_S4_ACT, T_POOL, T_UPSAMPLE, T_CE,
    T_UPSAMPLE_BWD, T_POOL_BWD, T_BN_BWD, T_BIAS_BWD, T_ZERO_STUFF, T_WGRAD, T_WAIT_WG, T_FORK, T_WG_DONE };
struct TCopyArgs { void *dst; const void *src; size_t bytes; };       // copy; zero fill (src unused)
struct TOneHotArgs { const void *seg; int seg_i64; const float *depth; const uint8_t *mask; float mean, stdv; int T, n_cls, H, W; float *x; };
struct TPackArgs { const float *theta; float *arena; const void *jobs; int n; };   // PackJob / S4WJob list
struct TZeroChArgs { float *t; int ctotal, c0, n; long long hw; };
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
struct TWgradArgs { const float *dy; float *partial, *dw; };
struct TStep {
    TStepKind kind;
    uint8_t stats;       // bit k: the step counts in pf_train_path_stats slot k
    int side, slot;      // side stream of the step (-1: the caller's stream); the dy slot of fork / wait_wg / wg_done
    ConvArgs a;          // conv_dma, conv_s4, pad_gather (the ranges it gathers), wgrad (the forward conv)
    int ks, stride, wm, nt;   // conv_dma: wm x nt (measure: chosen at enqueue); wgrad: ks, stride
    S4Shape s4;          // conv_s4: the instantiation that runs
    int Wp;              // pad_gather: the pitch of the gathered copy and where it goes
    float *gather;
    char tag[64];        // wgrad: profile tag of its launches (set when profiling)
    union {
        TCopyArgs copy; TOneHotArgs onehot; TPackArgs pack; TZeroChArgs zch; TUnpadArgs unpad; TUnpadMultiArgs unpadm; TBnFwdArgs bnf;
        TS4ActArgs s4act; TPlainArgs plain; TCeArgs ce; TUpBwdArgs upb; TBnBwdArgs bnb; TWgradArgs wg;
    } u;
};

std::array<int, 8> tune_key(const ConvArgs &c, int ks, int stride, int B) { return {ks, stride, c.Cin, c.Cout, c.Hin, c.Win, B, c.accum}; }

// pf_train_autotune, T_CONV_DMA_MEASURE: the workgroup shape of this geometry is measured unless an earlier conv of the pass did:
// every candidate of conv_dma's shape list, 1 warm-up + 3 timed launches; candidate (0, 0) = the cost model's own choice, kept
// unless a forced shape is at least 3 % faster.  Then the conv itself, with the shape kept
int tune_conv_dma(const pf_train *p, const ConvArgs &c, int ks, int stride, int B, hipStream_t s) {
    const std::array<int, 8> key = tune_key(c, ks, stride, B);
    auto it = p->tuned.find(key);
    if (it == p->tuned.end()) {
        if (!p->tune_ev[0] && (hipEventCreate(&p->tune_ev[0]) != hipSuccess || hipEventCreate(&p->tune_ev[1]) != hipSuccess))
            return fail(PF_EHIP, "autotune: hipEventCreate failed");
        float model_ms = 0.f, best = 1e30f;
        std::pair<int, int> pick{0, 0};
        const int wms[4] = {0, 4, 2, 1};
        for (int wi = 0; wi < 4; ++wi) {
            const int wm = wms[wi], ntmax = wm == 0 ? 1 : (wm == 1 ? 2 : 4);
            for (int nt = 1; nt <= ntmax && (wm == 0 || nt <= c.ntiles); ++nt) {
                int swm, snt;
                if (wm && !conv_dma_supported(c, ks, stride, B, wm, nt, 0, &swm, &snt)) continue;
                for (int rep = 0; rep < 4; ++rep) {      // 1 warm-up + 3 timed
                    if (rep == 1) PF_HIP_CHECK(hipEventRecord(p->tune_ev[0], s));
                    const int rc = wm ? launch_conv_dma(c, ks, stride, B, s, wm, nt) : launch_conv_dma(c, ks, stride, B, s);
                    if (rc) return rc;
                }
                PF_HIP_CHECK(hipEventRecord(p->tune_ev[1], s));
                PF_HIP_CHECK(hipEventSynchronize(p->tune_ev[1]));
                float ms = 0.f;
                PF_HIP_CHECK(hipEventElapsedTime(&ms, p->tune_ev[0], p->tune_ev[1]));
                if (!wm) model_ms = ms;
                else if (ms < best) best = ms, pick = {wm, nt};
            }
        }
        if (!(best < 0.97f * model_ms)) pick = {0, 0};
        it = p->tuned.emplace(key, pick).first;
    }
    return it->second.first ? launch_conv_dma(c, ks, stride, B, s, it->second.first, it->second.second) : launch_conv_dma(c, ks, stride, B, s);
}

// conv `c` reading ONE source instead of its ranges: all `cin` channels of buffer x, rows of `win` pixels (the gathered copy of an
// odd-width conv, the backward-data convs over dy)
ConvArgs over_buffer(ConvArgs c, const float *x, int cin, int win, int wout) {
    const BlobSrc all{0, 0, (uint32_t)cin};
    set_sources(c, order_plain(&all, 1), [&](uint32_t) { return TensorRef{x, cin}; });
    c.Cin = cin; c.Win = win; c.Wout = wout;
    return c;
}

// The whole step (input, weight packings, gradient clears, forward, loss, backward) into `steps`, every argument resolved into
// the call's theta, gradient and workspace.  Kernel choices are made here, through predicates: a geometry without a kernel
// fails before anything is enqueued.  measuring: the autotune pass - a conv_dma geometry this plan has not measured is measured
// at enqueue time (T_CONV_DMA_MEASURE)
int build_train_schedule(const pf_train *p, const TCall &k, const std::vector<Dims> &d, const TLayout &L, const GradFirst &gfirst,
                         bool measuring, std::vector<TStep> &steps) {
    // the options read per call
    const int kacc = g_opt_train_kacc, use_tuned = g_plan_opt.use_tuned_table, table_batch = g_opt_train_table_batch;
    const bool tagged = prof_enabled();
    const int B = k.B;
    char *wsb = (char *)k.ws;
    auto buf = [&](size_t off) { return reinterpret_cast<float *>(wsb + off); };
    auto act = [&](uint32_t t) { return buf(L.act[t]); };
    auto act_ref = [&](uint32_t t) { return TensorRef{act(t), (int)p->net.tensors[t].channels}; };
    auto gradt = [&](uint32_t t) { return buf(L.grad[t]); };
    const uint32_t input = p->net.ops[0].src[0].tensor;
    const int in_ch = (int)p->net.tensors[input].channels, n_cls = (int)p->net.hdr.n_cls;
    float *dy_slot[pf_train::kDySlots];
    for (int j = 0; j < pf_train::kDySlots; ++j) dy_slot[j] = buf(p->side && j ? L.dy_more[j] : L.dy);
    float *wpk_arena = buf(L.wpk_arena), *pad_in = buf(L.pad_in), *pad_out = buf(L.pad_out), *dfull = buf(L.dfull);
    float *up_tmp = g_opt_up_two_pass ? buf(L.up_tmp) : nullptr;
    double *cepart = reinterpret_cast<double *>(wsb + L.cepart), *bnpart = reinterpret_cast<double *>(wsb + L.bnpart);
    double *loss3 = reinterpret_cast<double *>(wsb + L.out3);
    steps.clear();
    auto add = [&](TStepKind kind, uint8_t stats = 0, int side = -1, int slot = 0) -> TStep & {
        TStep &st = steps.emplace_back();     // (zero-initialised)
        st.kind = kind; st.stats = stats; st.side = side; st.slot = slot;
        return st;
    };
    auto conv_args = [&](const BlobOp &o, const Dims &in, const Dims &out) {
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        set_sources(a, order_plain(o.src, (int)o.n_src), act_ref);
        a.bias = a.zero_page = p->dev_zero;
        a.Cin = (int)o.cin; a.Cout = (int)o.cout; a.ntiles = ((int)o.cout + 15) / 16;
        a.Hin = in.h; a.Win = in.w; a.Hout = out.h; a.Wout = out.w;
        return a;
    };
    // backward-data conv: `ch` gradient channels into dst from the cout_f channels of dy ([B][cout_f][h][w])
    auto bwd_data_args = [&](const float *dy, int cout_f, int ch, int h, int w, float *dst, int dst_ctotal, int dst_choff, int accum) {
        ConvArgs b;
        memset(&b, 0, sizeof(b));
        b.bias = b.zero_page = p->dev_zero;
        b.dst = dst; b.dst_ctotal = dst_ctotal; b.dst_choff = dst_choff; b.accum = accum;
        b.Cout = ch; b.Hin = h; b.Hout = h; b.ntiles = (ch + 15) / 16;
        return over_buffer(b, dy, cout_f, w, w);
    };
    // conv_dma over c with the tiled packing `job` and the measured shape of its geometry (autotune), else the table's row, else
    // the cost model's (path stats 2 / 0 / 1)
    auto dma = [&](ConvArgs c, int ks, int stride, int job, uint8_t stats) -> int {
        const PackJob &q = L.jobs[job];
        if (q.n_src != c.n_src) return fail(PF_EUNSUPPORTED, "training: a conv reads %d ranges, its weight packing %d", c.n_src, q.n_src);
        c.wpk = wpk_arena + q.out_off;
        c.nchunks = set_chunks(c, dma_kc(ks, stride)); c.rem = 0;
        c.kacc = (kacc && ks == 3) ? 1 : 0;     // blocked summation in the 3x3 convolutions (conv_dma.hip: KACC; option train_blocked_sum)
        const std::array<int, 8> key = tune_key(c, ks, stride, B);
        int wm = 0, nt = 0, src = 1;
        const auto it = p->autotune ? p->tuned.find(key) : p->tuned.end();
        if (forced_dma_shape(&wm, &nt)) {
            // pf_debug_force_conv(1, wm, nt, 0): every conv_dma step of the schedule with that shape (conv_dma_supported clamps nt to
            // the layer's cout tiles); counted in none of the path statistics' table / cost-model / measured slots
            src = 3;
        } else if (it != p->tuned.end()) {
            wm = it->second.first, nt = it->second.second, src = 2;
        } else if (measuring) {
            src = 2;
        } else if (use_tuned) {
            // option "train_table_batch" = n > 0: look the table up as if the batch were n (the rows are keyed on the batch they
            // were measured at; a parity test of the timed configuration's kernels on a batch the CPU oracle can afford pins n = 8)
            std::array<int, 8> tkey = key;
            if (table_batch > 0) tkey[6] = table_batch;
            for (const TrainTuned &t : kTrainTuned)
                if (t.wm && std::equal(tkey.begin(), tkey.end(), t.key)) {
                    wm = t.wm, nt = t.nt, src = 0;
                    break;
                }
        }
        TStep &st = add(src == 2 && it == p->tuned.end() ? T_CONV_DMA_MEASURE : T_CONV_DMA, stats | (uint8_t)(src < 3 ? 1u << src : 0u));
        st.a = c; st.ks = ks; st.stride = stride;
        if (st.kind == T_CONV_DMA && !conv_dma_supported(c, ks, stride, B, wm, nt, 0, &st.wm, &st.nt))
            return fail(PF_EUNSUPPORTED, "training: conv_dma has no kernel for ks=%d stride=%d wm=%d nt=%d", ks, stride, st.wm, st.nt);
        return PF_OK;
    };
    // the gathered, row-padded copy of the input ranges of `a` (path stats 3; 4: the conv keeps its output in padded rows)
    auto pad_gather = [&](const ConvArgs &a, int Wp, float *to, bool keep_padded) {
        TStep &st = add(T_PAD_GATHER, keep_padded ? 0x18 : 0x08);
        st.a = a; st.Wp = Wp; st.gather = to;
    };
    // one convolution on conv_dma.  Odd width: the same kernel on the input ranges gathered into `gather` with rows padded to a
    // multiple of 4; the output left in padded rows at a.dst (keep_padded: the BatchNorm kernels read that pitch) or scattered
    // back from pad_out
    auto conv = [&](const ConvArgs &a, int ks, int stride, int job, float *gather, bool keep_padded) -> int {
        if ((a.Win & 3) == 0) return dma(a, ks, stride, job, 0);
        const int Wp = (a.Win + 3) / 4 * 4, Wop = (Wp + 2 * (ks / 2) - ks) / stride + 1;
        pad_gather(a, Wp, gather, keep_padded);
        ConvArgs c = over_buffer(a, gather, a.Cin, Wp, Wop);
        c.dst = keep_padded ? a.dst : pad_out; c.dst_ctotal = a.Cout; c.dst_choff = 0; c.accum = 0;
        const int rc = dma(c, ks, stride, job, 0);
        if (rc || keep_padded) return rc;
        add(T_UNPAD).u.unpad = {pad_out, a.Cout, a.Hout, a.Wout, Wop, a.dst, a.dst_ctotal, a.dst_choff, a.accum};
        return PF_OK;
    };
    // the packed-pair shadow of channels [c0, c1) of tensor t, for the convolutions that read it through conv_s4
    // (a slice that starts or ends in the middle of a 4-channel group also zero-fills the group's other half while no producer has
    //  written it in this pass: a reader of this slice multiplies those channels by zero weights, and 0 x a stale NaN pattern is NaN)
    std::vector<std::vector<char>> s4_written(p->net.tensors.size());
    auto shadow = [&](uint32_t t, int c0, int c1) {
        if (L.s4act[t] == (size_t)-1) return;
        const int ct = (int)p->net.tensors[t].channels;
        std::vector<char> &wr = s4_written[t];
        if (wr.empty()) wr.assign((size_t)ct + 4, 0);
        const int fill_lo = (c0 & 2) && !wr[c0 - 2], fill_up = (c1 & 3) == 2 && c1 < ct && !wr[c1];
        for (int c = c0; c < c1; ++c) wr[c] = 1;
        add(T_S4_ACT).u.s4act = {act(t), ct, c0, c1, fill_lo, fill_up, d[t].h, d[t].w, (d[t].w + 3) / 4 * 4, wsb + L.s4act[t]};
    };
    int rc;

    // ---- input tensor (bg_model.py:61-69), weight packings (theta does not move inside this call), gradient clears
    if (k.x_dense) {
        add(T_COPY).u.copy = {act(input), k.x_dense, (size_t)B * in_ch * k.H * k.W * sizeof(float)};
    } else {
        if (k.T * (n_cls + 1) != in_ch) return fail(PF_EINVAL, "T=%d frames x (%d classes + depth) != %d input channels", k.T, n_cls, in_ch);
        add(T_ONEHOT).u.onehot = {k.seg, k.seg_is_i64, k.depth, k.depth_mask, k.depth_mean, k.depth_std, k.T, n_cls, k.H, k.W, act(input)};
    }
    add(T_PACK_TILED).u.pack = {k.theta, wpk_arena, L.jobs.data(), (int)L.jobs.size()};
    if (!L.s4jobs.empty()) add(T_PACK_S4).u.pack = {k.theta, buf(L.s4w_arena), L.s4jobs.data(), (int)L.s4jobs.size()};
    for (const auto &c : gfirst.clear)     // (no cleared gradient arena: first writers store)
        add(T_ZERO_CHANNELS).u.zch = {gradt((uint32_t)c[0]), (int)p->net.tensors[c[0]].channels, c[1], c[2], (long long)d[c[0]].h * d[c[0]].w};
    if (!k.accumulate_grads) add(T_ZERO_FILL).u.copy = {k.grad, nullptr, p->n_params * sizeof(float)};

    // ================================================================ forward (training mode)
    for (size_t i = 0; i < p->net.ops.size(); ++i) {
        const BlobOp &o = p->net.ops[i];
        const Dims in = d[o.src[0].tensor];
        const Dims out = o.kind == OP_HEAD ? in : d[o.dst];
        if (o.kind == OP_STEM || o.kind == OP_CONV) {
            ConvArgs a = conv_args(o, in, out);
            float *gather = L.odd[i] ? buf(L.xpad[i]) : pad_in;     // (an odd op keeps its copy for the weight gradient)
            const int Wp = (in.w + 3) / 4 * 4;
            if (!p->bn[i]) {
                a.bias = k.theta + p->aux_off[i];
                a.dst = act(o.dst); a.dst_ctotal = (int)p->net.tensors[o.dst].channels; a.dst_choff = (int)o.dst_choff; a.relu = (int)o.relu;
                if ((rc = conv(a, (int)o.k, (int)o.stride, L.fwd_job[i], gather, false))) return rc;
                shadow(o.dst, (int)o.dst_choff, (int)o.dst_choff + (int)o.cout);
                continue;
            }
            float *y = buf(L.ypre[i]);
            a.dst = y; a.dst_ctotal = (int)o.cout; a.dst_choff = 0; a.relu = 0;
            if (L.s4_job[i] < 0) {
                if ((rc = conv(a, (int)o.k, (int)o.stride, L.fwd_job[i], gather, L.odd[i]))) return rc;
            } else {
                // train_s4.hip: conv_s4 on the shadows of the input ranges; y in fp32 (rows padded to 4 on an odd-width level, as
                // the tiled fp32 path leaves them).  The weight gradient of an odd-width layer still reads the gathered, row-padded
                // fp32 copy of x
                const S4WJob &jb = L.s4jobs[L.s4_job[i]];
                if (L.odd[i]) pad_gather(a, Wp, gather, true);
                ConvArgs c = a;
                set_sources(c, order_plain(o.src, (int)o.n_src), [&](uint32_t t) { return TensorRef{buf(L.s4act[t]), (int)p->net.tensors[t].channels}; });
                c.src_fmt = 1; c.dst_fmt = 0;
                c.Win = Wp; c.Wout = Wp;
                c.acc_scale = 1.0f / (kS4TrainWeightScale * kS4TrainActScale);
                c.wpk = buf(L.s4w_arena) + jb.out_off;
                c.nchunks = jb.rounds;
                set_s4_entries(c, (int)o.k, jb.pad);
                c.kacc = (kacc && o.k == 3) ? 1 : 0;      // blocked summation, as in the fp32 step (conv_s4_kernel.inc: KACC)
                TStep &st = add(T_CONV_S4, 0x80);
                st.a = c; st.ks = (int)o.k;
                int nt = c.ntiles == 3 ? 3 : (c.ntiles < 2 ? 1 : 2), tile = S4_8x32;   // unless the layer's measured row names a shape
                ConvChoice row;
                if (use_tuned && choose_s4((int)o.k, c.Cin, c.Cout, c.Hout, c.Wout, B, &row) && row.is(CONV_S4)) { nt = row.s4_nt(); tile = row.s4_tile(); }
                st.s4 = s4_resolve(st.ks, nt, tile, c.ntiles, c.nchunks, c.kacc != 0);
            }
            float *aux = k.theta + p->aux_off[i], *stat = buf(L.stat[i]);
            add(T_BN_FWD).u.bnf = {y, (int)o.cout, out.h, out.w, k.bn_eps, k.bn_momentum, aux, aux + o.cout,
                                   k.update_running_stats ? aux + 2 * o.cout : nullptr, k.update_running_stats ? aux + 3 * o.cout : nullptr,
                                   stat, stat + o.cout, bnpart, act(o.dst), (int)p->net.tensors[o.dst].channels, (int)o.dst_choff, (int)o.relu,
                                   L.odd[i] ? (out.w + 3) / 4 * 4 : 0};
            shadow(o.dst, (int)o.dst_choff, (int)o.dst_choff + (int)o.cout);
        } else if (o.kind == OP_POOL) {
            add(T_POOL).u.plain = {act(o.src[0].tensor), act(o.dst), B * (int)o.cin, in.h, in.w, 0, 0, 0};
            shadow(o.dst, 0, (int)p->net.tensors[o.dst].channels);
        } else if (o.kind == OP_UPSAMPLE) {
            add(T_UPSAMPLE).u.plain = {act(o.src[0].tensor), act(o.dst), B * (int)o.cin, in.h, in.w, out.h, out.w, 0};
            shadow(o.dst, 0, (int)p->net.tensors[o.dst].channels);
        } else if (o.kind == OP_HEAD) {
            add(T_CE).u.ce = {act(o.src[0].tensor), (int)o.cin, in.h, in.w, k.labels, k.labels_i64, k.out_h, k.out_w, k.ignore_index, dfull, cepart, loss3};
            add(T_COPY).u.copy = {k.out3, loss3, 3 * sizeof(double)};
        }
    }

    // ================================================================ backward
    // With the side streams: layer n's conv-output gradient goes to dy slot n % kDySlots; the weight gradient (and its padded
    // copy of x) reads it on side stream n % kSideStreams while the caller's stream goes on to the input gradients and the next
    // layers; before it overwrites a slot it waits for the weight gradient of layer n - kDySlots that last read it.
    int n_conv = 0;
    for (size_t ii = p->net.ops.size(); ii-- > 0;) {
        const BlobOp &o = p->net.ops[ii];
        const Dims in = d[o.src[0].tensor];
        const Dims out = o.kind == OP_HEAD ? in : d[o.dst];
        const int store = gfirst.store[ii][0];
        if (o.kind == OP_HEAD) {
            // d loss / d logits = bilinear^T (softmax - onehot) * loss_scale / n_valid   (mean over the valid pixels, bg_model.py:81)
            add(T_UPSAMPLE_BWD).u.upb = {dfull, B * (int)o.cin, in.h, in.w, k.out_h, k.out_w, loss3 + 1, k.loss_scale, !store, gradt(o.src[0].tensor), up_tmp};
        } else if (o.kind == OP_POOL) {
            add(T_POOL_BWD).u.plain = {gradt(o.dst), gradt(o.src[0].tensor), B * (int)o.cin, in.h, in.w, 0, 0, store};
        } else if (o.kind == OP_UPSAMPLE) {
            add(T_UPSAMPLE_BWD).u.upb = {gradt(o.dst), B * (int)o.cin, in.h, in.w, out.h, out.w, nullptr, 1.f, !store, gradt(o.src[0].tensor), up_tmp};
        } else if (o.kind == OP_STEM || o.kind == OP_CONV) {
            if (!p->bn[ii] && o.relu) return fail(PF_EUNSUPPORTED, "training: ReLU without BatchNorm (op %zu)", ii);
            const int t_ctotal = (int)p->net.tensors[o.dst].channels;
            float *aux = k.theta + p->aux_off[ii], *gaux = k.grad + p->aux_off[ii];
            const int slot = n_conv % pf_train::kDySlots, sidx = n_conv % pf_train::kSideStreams;
            float *dy = dy_slot[slot];
            // odd-width levels: dy goes out with its rows padded to a multiple of 4 floats and zero pad columns - the form the
            // tiled weight-gradient and backward-data kernels read - and ONE backward-data conv covers all input ranges
            const bool odd = L.odd[ii];
            const int Wp = (in.w + 3) / 4 * 4, pitch = odd ? Wp : 0;
            if (p->side && n_conv >= pf_train::kDySlots) add(T_WAIT_WG, 0, -1, slot);
            ++n_conv;
            if (p->bn[ii]) {
                const float *stat = buf(L.stat[ii]);
                add(T_BN_BWD).u.bnb = {gradt(o.dst), t_ctotal, (int)o.dst_choff, buf(L.ypre[ii]), stat, stat + o.cout, aux, aux + o.cout,
                                       (int)o.cout, out.h, out.w, (int)o.relu, gaux, gaux + o.cout, bnpart, dy, pitch, pitch};
            } else {
                add(T_BIAS_BWD).u.bnb = {gradt(o.dst), t_ctotal, (int)o.dst_choff, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         (int)o.cout, out.h, out.w, 0, gaux, nullptr, bnpart, dy, pitch, 0};
            }
            // dW (odd width: the tiled kernel on the padded copy of x the forward pass gathered and the padded dy; zero pad
            // columns add nothing)
            if (p->side) add(T_FORK, 0, sidx, slot);
            {
                TStep &st = add(T_WGRAD, 0, p->side ? sidx : -1);
                const ConvArgs a = conv_args(o, in, out);
                st.a = odd ? over_buffer(a, buf(L.xpad[ii]), (int)o.cin, Wp, Wp) : a;
                st.ks = (int)o.k; st.stride = odd ? 1 : (int)o.stride;
                st.u.wg = {dy, buf(p->side && sidx ? L.wpart_more[sidx] : L.wpart), k.grad + p->w_off[ii]};
                if (tagged)      // per-layer rows of tools/bench_train.py --layers
                    snprintf(st.tag, sizeof(st.tag), "%02d %u->%u k%u s%u %dx%d", (int)ii, o.cin, o.cout, o.k, o.stride, out.h, out.w);
            }
            if (p->side) add(T_WG_DONE, 0, sidx, slot);
            // dX per input range (the network input needs none)
            const float *dsrc = dy;
            if (o.stride == 2) {
                float *up = dy + align_up((size_t)B * o.cout * out.h * out.w * sizeof(float), 256) / sizeof(float);
                bool needed = false;
                for (uint32_t j = 0; j < o.n_src; ++j) needed = needed || o.src[j].tensor != input;
                if (needed) add(T_ZERO_STUFF).u.plain = {dy, up, B * (int)o.cout, out.h, out.w, in.h, in.w, 0};
                dsrc = up;
            }
            if (odd) {
                const ConvArgs b = bwd_data_args(dy, (int)o.cout, (int)o.cin, in.h, Wp, pad_out, (int)o.cin, 0, 0);
                if ((rc = dma(b, (int)o.k, 1, L.bwd_all_job[ii], 0x20))) return rc;
                // one scatter launch for all ranges - unless two of them overlap in one tensor (an earlier range stores what a
                // later one adds to: they must not share a launch): then one launch per range, in range order
                bool overlap = false;
                for (uint32_t j = 0; j < o.n_src; ++j)
                    for (uint32_t j2 = 0; j2 < j; ++j2)
                        overlap = overlap || (o.src[j].tensor == o.src[j2].tensor && o.src[j].choff < o.src[j2].choff + o.src[j2].ch &&
                                              o.src[j2].choff < o.src[j].choff + o.src[j].ch);
                for (uint32_t only = 0; only < (overlap ? o.n_src : 1u); ++only) {
                    TUnpadMultiArgs &m = add(T_UNPAD_MULTI).u.unpadm;
                    m = {pad_out, (int)o.cin, in.h, in.w, Wp, (int)o.n_src, {}, {}, {}, {}, {}};
                    for (uint32_t j = 0; j < o.n_src; ++j) {
                        m.dst[j] = o.src[j].tensor != input && (!overlap || j == only) ? gradt(o.src[j].tensor) : nullptr;
                        m.ctotal[j] = (int)p->net.tensors[o.src[j].tensor].channels;
                        m.choff[j] = (int)o.src[j].choff;
                        m.ch[j] = (int)o.src[j].ch;
                        m.overwrite[j] = gfirst.store[ii][j];
                    }
                }
                continue;
            }
            for (uint32_t j = 0; j < o.n_src; ++j) {
                const uint32_t t = o.src[j].tensor;
                if (t == input) continue;
                const ConvArgs b = bwd_data_args(dsrc, (int)o.cout, (int)o.src[j].ch, in.h, in.w, gradt(t), (int)p->net.tensors[t].channels,
                                                 (int)o.src[j].choff, gfirst.store[ii][j] ? 0 : 1);
                if ((rc = conv(b, (int)o.k, 1, L.bwd_job[ii][j], pad_in, false))) return rc;
            }
        }
    }
    return PF_OK;
}

// One pass of a step: its schedule, then the enqueue loop - one launch or stream operation per step
// (measuring: the autotune pass - into the scratch gradient L.tune_grad, theta's running statistics left alone)
int train_pass(const pf_train *p, TCall k, bool measuring) {
    if (!p || !k.theta || !k.grad || !k.labels || !k.out3 || !k.ws) return fail(PF_EINVAL, "pf_train_forward_backward: null pointer argument");
    if (!k.x_dense && (!k.seg || !k.depth || !k.depth_mask)) return fail(PF_EINVAL, "pf_train_forward_backward: pass seg+depth+depth_mask or x_dense");
    if (k.B <= 0 || k.H <= 0 || k.W <= 0 || k.out_h <= 0 || k.out_w <= 0) return fail(PF_EINVAL, "pf_train_forward_backward: bad dims");
    std::vector<Dims> d;
    int rc = propagate_dims(p->net, k.H, k.W, d);
    if (rc) return rc;
    const TLayout L = t_layout(p, k.B, d, k.out_h, k.out_w);
    if (k.ws_bytes < L.total) return fail(PF_EWORKSPACE, "workspace %zu B < required %zu B", k.ws_bytes, L.total);
    if (measuring) {
        k.grad = reinterpret_cast<float *>((char *)k.ws + L.tune_grad);
        k.accumulate_grads = 0;
        k.update_running_stats = 0;
    }
    for (int &v : p->stats) v = 0;
    static thread_local std::vector<TStep> steps;     // (its storage is reused from call to call)
    if ((rc = build_train_schedule(p, k, d, L, grad_first_writers(p, d), measuring, steps))) return rc;
    for (const TStep &st : steps)
        for (int j = 0; j < 8; ++j) p->stats[j] += (st.stats >> j) & 1;
    // Every exit of this function - an error return in the middle of the backward pass included - leaves the side streams
    // JOINED to the caller's stream: a fork that is never joined invalidates an enclosing stream capture and lets the caller's
    // stream run ahead of weight gradients still in flight.
    struct SideJoin {
        const pf_train *p;
        hipStream_t s;
        int forked = 0;         // number of layers handed to the side streams so far
        bool done = false;
        int join() {
            if (done || !p->side || forked == 0) return PF_OK;
            done = true;
            for (int k = 0; k < pf_train::kSideStreams && k < forked; ++k) {   // (a stream that got no layer was never forked)
                PF_HIP_CHECK(hipEventRecord(p->ev_join[k], p->sides[k]));
                PF_HIP_CHECK(hipStreamWaitEvent(s, p->ev_join[k], 0));
            }
            return PF_OK;
        }
        ~SideJoin() { (void)join(); }
    } side_join{p, k.s};
    const hipStream_t s = k.s;
    const int B = k.B;
    for (const TStep &st : steps) {
        const hipStream_t ss = st.side >= 0 ? p->sides[st.side] : s;
        const auto &u = st.u;
        switch (st.kind) {
            case T_COPY: rc = launch_copy(u.copy.dst, u.copy.src, u.copy.bytes, s); break;
            case T_ONEHOT: { const TOneHotArgs &x = u.onehot;
                rc = launch_onehot_dense(x.seg, x.seg_i64, x.depth, x.mask, x.mean, x.stdv, B, x.T, x.n_cls, x.H, x.W, x.x, s); break; }
            case T_PACK_TILED: rc = launch_pack_weights_batch(u.pack.theta, u.pack.arena, (const PackJob *)u.pack.jobs, u.pack.n, s); break;
            case T_PACK_S4: rc = launch_s4_pack_weights_dev(u.pack.theta, u.pack.arena, (const S4WJob *)u.pack.jobs, u.pack.n, kS4TrainWeightScale, s); break;
            case T_ZERO_CHANNELS: rc = launch_zero_channels(u.zch.t, B, u.zch.ctotal, u.zch.c0, u.zch.n, u.zch.hw, s); break;
            case T_ZERO_FILL: rc = launch_zero_fill(u.copy.dst, u.copy.bytes, s); break;
            case T_PAD_GATHER: rc = launch_pad_gather(st.a, B, st.Wp, st.gather, s); break;
            case T_CONV_DMA: rc = launch_conv_dma(st.a, st.ks, st.stride, B, s, st.wm, st.nt); break;
            case T_CONV_DMA_MEASURE: rc = tune_conv_dma(p, st.a, st.ks, st.stride, B, s); break;
            case T_CONV_S4: rc = launch_conv_s4(st.a, st.ks, st.s4, B, s); break;
            case T_UNPAD: { const TUnpadArgs &x = u.unpad;
                rc = launch_unpad_scatter(x.src, B, x.C, x.H, x.W, x.Wp, x.dst, x.ctotal, x.choff, x.accum, s); break; }
            case T_UNPAD_MULTI: { const TUnpadMultiArgs &x = u.unpadm;
                rc = launch_unpad_scatter_multi(x.src, B, x.C, x.H, x.W, x.Wp, x.dst, x.ctotal, x.choff, x.ch, x.overwrite, x.n, s); break; }
            case T_BN_FWD: { const TBnFwdArgs &x = u.bnf;
                rc = launch_bn_forward(x.y, B, x.C, x.H, x.W, x.eps, x.momentum, x.gamma, x.beta, x.rmean, x.rvar, x.mean, x.invstd, x.part,
                                       x.dst, x.dst_ctotal, x.dst_choff, x.relu, x.y_pitch, s); break; }
            case T_S4_ACT: { const TS4ActArgs &x = u.s4act;
                rc = launch_s4_pack_act(x.src, B, x.ctotal, x.c0, x.c1, x.fill_lo, x.fill_up, x.H, x.W, x.Wp, x.dst, kS4TrainActScale, s); break; }
            case T_POOL: rc = launch_avgpool2(u.plain.src, u.plain.dst, u.plain.planes, u.plain.hin, u.plain.win, nullptr, nullptr, s); break;
            case T_UPSAMPLE: { const TPlainArgs &x = u.plain;
                rc = launch_upsample(x.src, x.dst, x.planes, x.hin, x.win, x.hout, x.wout, nullptr, nullptr, s); break; }
            case T_CE: { const TCeArgs &x = u.ce;
                rc = launch_ce_fwd_bwd(x.logits, B, x.C, x.hi, x.wi, x.labels, x.lab_i64, x.ho, x.wo, x.ignore, x.dfull, x.part, x.out3, s); break; }
            case T_UPSAMPLE_BWD: { const TUpBwdArgs &x = u.upb;
                rc = launch_upsample_bwd(x.gout, x.planes, x.hi, x.wi, x.ho, x.wo, x.count, x.scale, x.accumulate, x.gin, x.tmp, s); break; }
            case T_POOL_BWD: rc = launch_avgpool2_bwd(u.plain.src, u.plain.planes, u.plain.hin, u.plain.win, u.plain.overwrite, u.plain.dst, s); break;
            case T_BN_BWD: { const TBnBwdArgs &x = u.bnb;
                rc = launch_bn_backward(x.g, x.t_ctotal, x.choff, x.y, x.mean, x.invstd, x.gamma, x.beta, B, x.C, x.H, x.W, x.relu, x.dgamma,
                                        x.dbeta, x.part, x.dy, x.dy_pitch, x.y_pitch, s); break; }
            case T_BIAS_BWD: { const TBnBwdArgs &x = u.bnb;
                rc = launch_bias_backward(x.g, x.t_ctotal, x.choff, B, x.C, x.H, x.W, x.dgamma, x.part, x.dy, x.dy_pitch, s); break; }
            case T_ZERO_STUFF: rc = launch_zero_stuff(u.plain.src, u.plain.planes, u.plain.hin, u.plain.win, u.plain.hout, u.plain.wout, u.plain.dst, s); break;
            case T_WGRAD:
                if (st.tag[0]) prof_set_tag(st.tag);
                rc = launch_wgrad(st.a, st.ks, st.stride, u.wg.dy, B, u.wg.partial, u.wg.dw, ss);
                if (st.tag[0]) prof_set_tag(nullptr);
                break;
            case T_WAIT_WG: PF_HIP_CHECK(hipStreamWaitEvent(s, p->ev_wg[st.slot], 0)); break;
            case T_FORK:
                PF_HIP_CHECK(hipEventRecord(p->ev_dy[st.slot], s));
                PF_HIP_CHECK(hipStreamWaitEvent(ss, p->ev_dy[st.slot], 0));
                ++side_join.forked;
                break;
            case T_WG_DONE: PF_HIP_CHECK(hipEventRecord(p->ev_wg[st.slot], ss)); break;
        }
        if (rc) return rc;
    }
    return side_join.join();   // the caller's stream carries every gradient when this call's work is done
}

}  // namespace

extern "C" int pf_train_forward_backward(const pf_train *p, float *theta, float *grad, int accumulate_grads, const void *seg, int seg_is_i64,
                                         const float *depth, const uint8_t *depth_mask, float depth_mean, float depth_std, int T,
                                         const float *x_dense, int B, int H, int W, const void *labels, int labels_i64, int out_h, int out_w,
                                         int ignore_index, float loss_scale, float bn_momentum, float bn_eps, int update_running_stats,
                                         double *out3, void *ws, size_t ws_bytes, void *stream) {
    const TCall k{theta, grad, accumulate_grads, seg, seg_is_i64, depth, depth_mask, depth_mean, depth_std, T, x_dense, B, H, W, labels, labels_i64,
                  out_h, out_w, ignore_index, loss_scale, bn_momentum, bn_eps, update_running_stats, out3, ws, ws_bytes, (hipStream_t)stream};
    if (p && p->autotune && ws) {
        // pf_train_autotune: the measurements run in a pass of their own in front of the first real pass of a configuration
        // (B, H, W, out_h, out_w) outside a capture: its launches repeat, so what they accumulate is garbage - it goes to a scratch
        // gradient and leaves theta alone
        const std::array<int, 5> cfg{B, H, W, out_h, out_w};
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        const bool seen = std::find(p->measured_configs.begin(), p->measured_configs.end(), cfg) != p->measured_configs.end();
        if (!seen && hipStreamIsCapturing(k.s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone) {
            const int rc = train_pass(p, k, true);
            if (rc) return rc;
            p->measured_configs.push_back(cfg);
        }
    }
    return train_pass(p, k, false);
}

extern "C" int pf_sgd_workspace(size_t *bytes) {
    if (!bytes) return fail(PF_EINVAL, "pf_sgd_workspace: null");
    *bytes = sgd_ws_bytes();
    return PF_OK;
}

extern "C" int pf_sgd_step(float *theta, float *grad, float *momentum_buf, const uint8_t *trainable, size_t n, float lr, float momentum,
                           float weight_decay, float clip_norm, float clip_value, int first_step, void *ws, size_t ws_bytes, void *stream) {
    if (!theta || !grad || !momentum_buf || !trainable || !ws || n == 0) return fail(PF_EINVAL, "pf_sgd_step: null argument");
    if (ws_bytes < sgd_ws_bytes()) return fail(PF_EWORKSPACE, "pf_sgd_step: workspace %zu B < required %zu B", ws_bytes, sgd_ws_bytes());
    return launch_sgd(theta, grad, momentum_buf, trainable, (long long)n, lr, momentum, weight_decay, clip_norm, clip_value, first_step, ws,
                      (hipStream_t)stream);
}
