// A forward of a plan (hardnet_plan.h; built by plan_create.hip) = build_schedule (hardnet_schedule.cpp: the op table -> a flat list
// of launches, every fusion and kernel choice made on the host) + the enqueue loop over it, here, with the two entry points.
#include <cstdlib>
#include <cstring>

#include "hardnet_schedule.h"
#include "pf_prof.h"

using namespace pf;

namespace {

// One launcher per step kind; the debugging switches (PF_SYNC_OPS, PF_PROBE: instrumented builds only) are read here and nowhere else
int run_net(const pf_plan *p, const StemArgs *stem, const float *dense_x, int B, int H, int W, int out_h, int out_w,
            void *out_seg, int out_seg_is_i64, float *out_logits, float *out_orig, void *ws, size_t ws_bytes,
            hipStream_t s) {
    std::vector<Step> steps;   // (per call: no state kept across forwards)
    std::vector<uint8_t> fmt;
    int rc = build_schedule(p, stem, dense_x, B, H, W, out_h, out_w, out_seg, out_seg_is_i64, out_logits, out_orig, ws, ws_bytes, steps, fmt);
    if (rc) return rc;
    p->last_fmt = fmt;
    static const bool sync_ops = ab_env("PF_SYNC_OPS") != nullptr;   // debugging: localise a faulting launch
    static const bool probe_on = ab_env("PF_PROBE") != nullptr;      // read once, not per forward
    long long *const probe = probe_on ? probe_buffer() : nullptr;
    for (size_t k = 0; k < steps.size(); ++k) {
        Step &st = steps[k];
        if (sync_ops && (k == 0 || steps[k - 1].op != st.op))
            fprintf(stderr, "[pf] before op %d (%s): %s\n", st.op, p->net.tensors[p->net.ops[st.op].dst].name, hipGetErrorString(hipStreamSynchronize(s)));
        else if (sync_ops && is_conv_step(steps[k - 1].kind) && steps[k - 1].u.c.no_bias)
            fprintf(stderr, "[pf]   low-resolution half: %s\n", hipGetErrorString(hipStreamSynchronize(s)));
        if (st.tag[0]) prof_set_tag(st.tag);
        const BlobOp &o = p->net.ops[st.ci];
        ConvArgs &a = st.u.c;   // (the conv kinds)
        const ConvChoice &ch = st.dec.ch;
        const PlainArgs &x = st.u.x;
        if (is_conv_step(st.kind)) a.probe = probe;
        switch (st.kind) {
            case S_RANGE_CHECK: rc = launch_range_check(x.src, x.n, x.status, x.slot, s); break;
            case S_STEM: st.u.sf.stem.probe = probe; rc = launch_stem(st.u.sf.stem, s); break;
            case S_STEM_FRONT:   // (conv_front under a label of its own)
                if ((rc = launch_stem(st.u.sf.stem, s))) break;
                if (st.u.sf.front_tag[0]) prof_set_tag(st.u.sf.front_tag);
                st.u.sf.front.probe = probe; rc = launch_conv_front(st.u.sf.front, B, s); break;
            case S_PAIR: st.u.pair.c.probe = probe; rc = launch_conv_pair(st.u.pair, B, s); break;
            case S_CONV_S4: rc = launch_conv_s4(a, (int)o.k, st.dec.s4, B, s); break;
            case S_CONV_S4_SHARE: rc = launch_conv_s4_share(a, st.dec.s4_nt, B, s); break;
            case S_CONV_S4_ADD: rc = launch_conv_s4_add(a, st.dec.s4_nt, B, s); break;
            case S_CONV_S4_TAIL: rc = launch_conv_s4_tail(a, B, s); break;
            case S_CONV_S4_DOWN: rc = launch_conv_s4_down(a, B, s); break;
            case S_CONV_S4_LO: rc = launch_conv_s4_lo(a, B, s); break;
            case S_CONV_GENERIC: rc = launch_conv(a, p->conv[st.ci].tiling, B, s); break;
            case S_CONV_SPLIT: rc = launch_conv_split(a, ch.split_nt(), ch.split_wide(), B, s); break;
            case S_CONV_SPLIT1: rc = launch_conv_split1(a, ch.split_nt(), B, s); break;
            case S_CONV_WAVE: rc = launch_conv_wave(a, (int)o.k, ch.wave_mh(), ch.wave_nt(), ch.wave_wk(), B, s); break;
            case S_CONV_DMA: rc = launch_conv_dma(a, (int)o.k, (int)o.stride, B, s, ch.dma_wm(), ch.dma_nt(), p->opt.table_batch); break;
            case S_POOL: rc = launch_avgpool2(x.src, x.dst, x.planes, x.hin, x.win, x.status, x.slot, s); break;
            case S_UPSAMPLE: rc = launch_upsample(x.src, x.dst, x.planes, x.hin, x.win, x.hout, x.wout, x.status, x.slot, s); break;
            case S_HEAD:
                if (st.u.head.orig && (rc = launch_copy(st.u.head.orig, st.u.head.h.logits, st.u.head.orig_bytes, s))) break;
                rc = launch_head(st.u.head.h, s); break;
            case S_CONV: break;   // (never left in a schedule)
        }
        if (rc) return rc;
    }
    if (p->opt.profile_tag_ops != 0 || g_plan_opt.profile_tag_ops != 0) prof_set_tag(nullptr);
    // the dense input's slot is the last word of the block: the finalizer scans all of it (unused slots stay 0)
    return launch_range_finalize(reinterpret_cast<unsigned *>(ws), kLiveWord, kSlot0, kMaxSlots, kStickyWord, s);
}

}  // namespace

extern "C" int pf_bg_forward(const pf_plan *p, const void *seg, int seg_is_i64, const float *depth,
                             const uint8_t *depth_mask, float depth_mean, float depth_std, int hop_flags,
                             float min_depth, float max_depth, int B, int T, int H, int W, int out_h, int out_w,
                             void *out_seg, int out_seg_is_i64, float *out_logits, float *out_orig_logits, void *ws,
                             size_t ws_bytes, void *stream) {
    if (!p || !seg || !depth || !out_seg || !ws) return fail(PF_EINVAL, "pf_bg_forward: null pointer argument");
    if (!depth_mask && !(hop_flags & PF_HOP_DEPTH_U16))
        return fail(PF_EINVAL, "pf_bg_forward: depth_mask is required unless PF_HOP_DEPTH_U16 is set");
    if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0)
        return fail(PF_EINVAL, "pf_bg_forward: bad dims");
    if (p->net.ops.empty() || p->net.ops[0].kind != OP_STEM)
        return fail(PF_EUNSUPPORTED, "pf_bg_forward: plan does not start with a fused stem");
    StemArgs st;
    memset(&st, 0, sizeof(st));
    st.seg = seg; st.depth = depth; st.mask = depth_mask;
    st.depth_mean = depth_mean; st.depth_std = depth_std; st.min_depth = min_depth; st.max_depth = max_depth;
    st.seg_is_i64 = seg_is_i64; st.hop = hop_flags; st.B = B; st.T = T; st.n_cls = (int)p->net.hdr.n_cls;
    st.H = H; st.W = W;
    return run_net(p, &st, nullptr, B, H, W, out_h, out_w, out_seg, out_seg_is_i64, out_logits, out_orig_logits, ws,
                   ws_bytes, (hipStream_t)stream);
}

extern "C" int pf_hardnet_forward_dense(const pf_plan *p, const float *x, int B, int H, int W, int out_h, int out_w,
                                        void *out_seg, int out_seg_is_i64, float *out_logits, float *out_orig_logits,
                                        void *ws, size_t ws_bytes, void *stream) {
    if (!p || !x || !ws) return fail(PF_EINVAL, "pf_hardnet_forward_dense: null pointer argument");
    if (B <= 0 || H <= 0 || W <= 0) return fail(PF_EINVAL, "pf_hardnet_forward_dense: bad dims");
    const bool has_head = !p->net.ops.empty() && p->net.ops.back().kind == OP_HEAD;
    if (has_head && (!out_seg || out_h <= 0 || out_w <= 0))
        return fail(PF_EINVAL, "pf_hardnet_forward_dense: out_seg/out size required");
    return run_net(p, nullptr, x, B, H, W, out_h, out_w, out_seg, out_seg_is_i64, out_logits, out_orig_logits, ws,
                   ws_bytes, (hipStream_t)stream);
}
