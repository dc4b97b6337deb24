// bg training step (scope row f4): forward in training mode + loss + backward over the op table, and the optimiser step.
//
// Replaces, for task `bg`, what the reference's training loop does per batch (training/train.py:185-222):
//     loss_dict = model.loss(inputs, labels)      models/bg/bg_model.py:73-89  (train-mode BatchNorm, F.interpolate, CrossEntropyLoss)
//     loss.backward()                             autograd through hardnet.py:353-387
//     clip_grad_value_ / clip_grad_norm_ ; opt.step()  (SGD, momentum, weight decay: train.py:130-138)
//
// A step = t_layout (train_layout.cpp: theta and the workspace) + build_train_schedule (train_schedule.cpp: the whole step as a flat
// list of TSteps) - host code only, shared through train_plan.h - + the enqueue loop of train_pass here, a switch with one call per
// step.  This file holds what needs the device: the plan object with its streams and events, the C API, the autotuner.
#include <algorithm>
#include <cstring>

#include "pf_prof.h"
#include "train_plan.h"

using namespace pf;

struct pf_train {
    TrainNet n;
    float *dev_zero = nullptr;            // 1024 zeros (the zero bias and zero page of the conv launches)
    // the weight gradients are leaves of the backward pass: they run on this plan's own lower-priority streams, forked from and
    // joined to the caller's stream inside every pf_train_forward_backward (so a stream capture of the call stays one graph).
    // Option "train_side_stream" (read when the plan is created: n.side; 0 = everything on the caller's stream)
    hipStream_t sides[kSideStreams] = {};
    hipEvent_t ev_dy[kDySlots] = {}, ev_wg[kDySlots] = {}, ev_join[kSideStreams] = {};
    // pf_train_autotune: the workgroup shape (pixel waves x cout tiles) of every forward / backward-data convolution is MEASURED
    // the first time its geometry is seen outside a stream capture (every candidate of conv_dma's shape list, 3 launches each,
    // hipEvents) instead of taken from the inference path's cost model, which was calibrated on 1024x2048 batches.  Off by default:
    // the choice (and with it the summation order of K-split shapes) then depends on timing, i.e. may differ from run to run.
    int autotune = 0;
    mutable TunedMap tuned;
    mutable hipEvent_t tune_ev[2] = {nullptr, nullptr};
    // pf_train_path_stats: which code paths the LAST pf_train_forward_backward took, counted from its schedule (tests assert that
    // a timed configuration really ran the table's shapes and the padded odd-width forms)
    mutable int stats[8] = {};
    mutable std::vector<std::array<int, 5>> measured_configs;
};

namespace pf {   // the process-wide switches of the training step (pf_set_option: plan_create.hip)
int g_opt_up_two_pass = 1;         // upsample_bwd_two_pass: the bilinear transposes of large planes as rows-then-columns passes (train_resample.hip)
int g_opt_train_table_batch = 0;   // train_table_batch: batch size the rows of train_tuned.inc are looked up with (0 = the call's own)
int g_opt_train_kacc = 1;          // train_blocked_sum: per-round partial sums in the 3x3 convolutions of a training step (conv_dma.hip: KACC)
int g_opt_train_s4 = 0;            // train_forward_s4: the forward convolutions of a training step on conv_s4 with blocked sums (train_s4.hip); opt-in
int g_opt_train_side = 1;          // train_side_stream: weight gradients on the training plan's own stream
}

extern "C" int pf_train_create(const void *blob, size_t bytes, int in_ch, int n_cls, pf_train **out) {
    if (!blob || !out) return fail(PF_EINVAL, "pf_train_create: null argument");
    pf_train *p = new pf_train();
    if (int rc = train_net_init(blob, bytes, in_ch, n_cls, p->n)) {
        delete p;
        return rc;
    }
    if (hipMalloc((void **)&p->dev_zero, 1024 * sizeof(float)) != hipSuccess || hipMemset(p->dev_zero, 0, 1024 * sizeof(float)) != hipSuccess) {
        delete p;
        return fail(PF_EHIP, "pf_train_create: device allocation failed");
    }
    if (p->n.side) {
        int lo = 0, hi = 0;
        bool ok = hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess;
        for (int k = 0; ok && k < kSideStreams; ++k) ok = hipStreamCreateWithPriority(&p->sides[k], hipStreamNonBlocking, lo) == hipSuccess;
        for (int k = 0; ok && k < kDySlots; ++k)
            ok = hipEventCreateWithFlags(&p->ev_dy[k], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&p->ev_wg[k], hipEventDisableTiming) == hipSuccess;
        for (int k = 0; ok && k < kSideStreams; ++k) ok = hipEventCreateWithFlags(&p->ev_join[k], hipEventDisableTiming) == hipSuccess;
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
    for (int k = 0; k < kDySlots; ++k) {
        if (p->ev_dy[k]) (void)hipEventDestroy(p->ev_dy[k]);
        if (p->ev_wg[k]) (void)hipEventDestroy(p->ev_wg[k]);
    }
    for (hipEvent_t e : p->tune_ev)
        if (e) (void)hipEventDestroy(e);
    for (int k = 0; k < kSideStreams; ++k) {
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
    *n_floats = p->n.n_params;
    return PF_OK;
}

extern "C" int pf_train_param_layout(const pf_train *p, int op_index, size_t *w_off, size_t *aux_off, int *has_bn) {
    if (!p || op_index < 0 || (size_t)op_index >= p->n.net.ops.size() || !w_off || !aux_off || !has_bn) return fail(PF_EINVAL, "pf_train_param_layout: bad argument");
    if (!is_conv(p->n.net.ops[op_index].kind)) return fail(PF_EINVAL, "op %d is not a convolution", op_index);
    *w_off = p->n.w_off[op_index];
    *aux_off = p->n.aux_off[op_index];
    *has_bn = p->n.bn[op_index];
    return PF_OK;
}

extern "C" int pf_train_workspace(const pf_train *p, int B, int H, int W, int out_h, int out_w, size_t *bytes) {
    if (!p || !bytes || B <= 0 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0) return fail(PF_EINVAL, "pf_train_workspace: bad argument");
    std::vector<Dims> d;
    int rc = propagate_dims(p->n.net, H, W, d);
    if (rc) return rc;
    *bytes = t_layout(p->n, p->autotune, B, d, out_h, out_w).total;
    return PF_OK;
}

extern "C" int pf_train_tensor_view(const pf_train *p, const char *name, int want_grad, int B, int H, int W, int out_h, int out_w,
                                    size_t *ws_offset, int *channels, int *h, int *w) {
    if (!p || !name || !ws_offset || !channels || !h || !w) return fail(PF_EINVAL, "pf_train_tensor_view: null");
    std::vector<Dims> d;
    int rc = propagate_dims(p->n.net, H, W, d);
    if (rc) return rc;
    const TLayout L = t_layout(p->n, p->autotune, B, d, out_h, out_w);
    const std::vector<BlobTensor> &tensors = p->n.net.tensors;
    for (size_t t = 0; t < tensors.size(); ++t)
        if (strncmp(tensors[t].name, name, sizeof(tensors[t].name)) == 0) {
            const size_t off = want_grad ? L.grad[t] : L.act[t];
            if (off == (size_t)-1) return fail(PF_EINVAL, "tensor '%s' has no %s buffer", name, want_grad ? "gradient" : "activation");
            *ws_offset = off; *channels = (int)tensors[t].channels; *h = d[t].h; *w = d[t].w;
            return PF_OK;
        }
    return fail(PF_EINVAL, "no tensor named '%s'", name);
}

namespace {

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

// One pass of a step: its schedule, then the enqueue loop - one launch or stream operation per step
// (measuring: the autotune pass - into the scratch gradient L.tune_grad, theta's running statistics left alone)
int train_pass(const pf_train *p, TCall k, bool measuring) {
    if (!p || !k.theta || !k.grad || !k.labels || !k.out3 || !k.ws) return fail(PF_EINVAL, "pf_train_forward_backward: null pointer argument");
    if (!k.x_dense && (!k.seg || !k.depth || !k.depth_mask)) return fail(PF_EINVAL, "pf_train_forward_backward: pass seg+depth+depth_mask or x_dense");
    if (k.B <= 0 || k.H <= 0 || k.W <= 0 || k.out_h <= 0 || k.out_w <= 0) return fail(PF_EINVAL, "pf_train_forward_backward: bad dims");
    std::vector<Dims> d;
    int rc = propagate_dims(p->n.net, k.H, k.W, d);
    if (rc) return rc;
    const TLayout L = t_layout(p->n, p->autotune, k.B, d, k.out_h, k.out_w);
    if (k.ws_bytes < L.total) return fail(PF_EWORKSPACE, "workspace %zu B < required %zu B", k.ws_bytes, L.total);
    if (measuring) {
        k.grad = reinterpret_cast<float *>((char *)k.ws + L.tune_grad);
        k.accumulate_grads = 0;
        k.update_running_stats = 0;
    }
    for (int &v : p->stats) v = 0;
    static thread_local std::vector<TStep> steps;     // (its storage is reused from call to call)
    if ((rc = build_train_schedule(p->n, k, d, L, grad_first_writers(p->n, d), p->dev_zero, p->autotune ? &p->tuned : nullptr, measuring, steps))) return rc;
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
            if (done || forked == 0) return PF_OK;
            done = true;
            for (int k = 0; k < kSideStreams && k < forked; ++k) {   // (a stream that got no layer was never forked)
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
            case T_PAD_GATHER: rc = launch_pad_gather(u.gather.a, B, u.gather.Wp, u.gather.dst, s); break;
            case T_CONV_DMA: rc = launch_conv_dma(u.conv.a, u.conv.ks, u.conv.stride, B, s, u.conv.wm, u.conv.nt); break;
            case T_CONV_DMA_MEASURE: rc = tune_conv_dma(p, u.conv.a, u.conv.ks, u.conv.stride, B, s); break;
            case T_CONV_S4: rc = launch_conv_s4(u.conv.a, u.conv.ks, u.conv.s4, B, s); break;
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
            case T_WGRAD: { const TWgradArgs &x = u.wg;
                if (x.tag[0]) prof_set_tag(x.tag);
                rc = launch_wgrad(x.a, x.ks, x.stride, x.dy, B, x.partial, x.dw, ss);
                if (x.tag[0]) prof_set_tag(nullptr);
                break; }
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
