// The schedule of an inference forward, host code only: build_schedule turns the plan's op table into the flat list of launches that
// hardnet_plan.hip enqueues - every fusion and every kernel choice made here, each step naming exactly one kernel with all its arguments.
// Six passes over one context (Sched): dims and workspace layout, the op walk with its fusions, the tensor formats, each convolution's
// kernel, pair / share-add, the folds.  It computes with the pointers it is given and reads nothing through them, so
// pf_debug_hardnet_schedule (below) builds the same schedule over made-up addresses and hands it to tests without a device.
//
// Replaces the module walk of reference hardnet.py:353-387 (hardnet.forward) and the glue of bg_model.py:61-71,91-102.  The op table
// comes from the blob (packing.py / hardnet_arch.py); nothing about FC-HarDNet-70 is hard-coded here, so single-op test networks use
// the same code.
#include <algorithm>
#include <cstring>

#include "hardnet_schedule.h"
#include "pf_prof.h"

namespace pf {

int layout(const pf_plan *p, int B, int H, int W, std::vector<Dims> &d, std::vector<size_t> &off, size_t &total, size_t *share_off) {
    int rc = propagate_dims(p->net, H, W, d);
    if (rc) return rc;
    off.assign(p->net.tensors.size(), (size_t)-1);
    size_t cur = kStatusBytes;
    const uint32_t input = p->net.ops[0].src[0].tensor;
    for (size_t t = 0; t < p->net.tensors.size(); ++t) {
        if (t == input || d[t].h == 0) continue;
        off[t] = cur;
        // channels padded to whole groups of 4: the same region holds the tensor as fp32 NCHW or in the S4 layout
        cur += align_up((size_t)B * ((p->net.tensors[t].channels + 3) / 4 * 4) * d[t].h * d[t].w * sizeof(float), 256);
    }
    // the stored sums of the share / add launches: fp32 units of four of the consumer's channels per pixel, sized for the largest pair
    // the plan's share_s option selects at this batch; the share launch's write and the add launch's read are adjacent steps of one
    // stream, so every pair uses the same region
    size_t share_bytes = 0;
    const int Bt = p->opt.table_batch > 0 ? p->opt.table_batch : B;
    for (size_t i = 1; i < p->net.ops.size(); ++i) {
        const BlobOp &P = p->net.ops[i - 1], &C = p->net.ops[i];
        const Dims &o = d[C.dst];
        if (p->conv[i].share_a_off && p->opt.share_s && share_wanted((int)P.cin, (int)P.cout, (int)C.cin, (int)C.cout, o.h, o.w, Bt, p->opt.share_s))
            share_bytes = std::max(share_bytes, (size_t)B * ((C.cout + 3) / 4 * 4) * o.h * o.w * sizeof(float));
    }
    if (share_off) *share_off = share_bytes ? cur : (size_t)-1;
    cur += align_up(share_bytes, 256);
    total = cur;
    return PF_OK;
}

namespace {

// What the passes of one build_schedule share: the call, the plan's geometry, the status words, the format bookkeeping, the steps
struct Sched {
    const pf_plan *p;
    const StemArgs *stem;
    const float *dense_x;
    int B, out_h, out_w;
    void *out_seg;
    int out_seg_is_i64;
    float *out_logits, *out_orig;
    void *ws;
    std::vector<Step> &steps;
    std::vector<uint8_t> &fmt;

    // pass 1
    std::vector<Dims> d;
    std::vector<size_t> off;
    size_t share_off = (size_t)-1;
    uint32_t input = 0;
    bool tags = false, fuse = false, fuse_up = false, s4_allowed = false;
    int Bt = 0;   // the batch every kernel choice is made for (option "table_batch")
    unsigned *st_words = nullptr, *status_all = nullptr;
    // Tensor formats: a tensor is S4 iff every step that reads it reads all its inputs as S4 and every step that writes it can
    // write S4.  cand = still possible; written = channels of each tensor some earlier step stores (half-group bookkeeping)
    std::vector<uint8_t> cand;
    std::vector<std::vector<uint8_t>> written;

    float *tptr(uint32_t t) const { return t == input ? const_cast<float *>(dense_x) : reinterpret_cast<float *>((char *)ws + off[t]); }
    TensorRef tref(uint32_t t) const { return TensorRef{tptr(t), (int)p->net.tensors[t].channels}; }
    // the guard of a launch: only if what it stores can become an operand of a split kernel (the logits cannot)
    unsigned *status_of(uint32_t dst_t) const { return p->feeds_conv[dst_t] ? status_all : nullptr; }
    unsigned *slot_of(size_t op_i, uint32_t dst_t) const { return (status_all && p->feeds_conv[dst_t]) ? st_words + kSlot0 + op_i : nullptr; }
    // a step stores channels [lo, hi) of tensor t: returns its S4 dst_limit (zero-fill the tail of the last group unless its owner
    // wrote it already)
    int claim(uint32_t t, int lo, int hi) {
        std::vector<uint8_t> &wr = written[t];
        if ((lo & 3) == 2 && !wr[lo - 2]) cand[t] = 0;   // would expose an unwritten half group to readers of this range
        const int limit = ((hi & 3) != 0 && !wr[hi]) ? (hi + 3) / 4 * 4 : hi;
        for (int c = lo; c < hi; ++c) wr[c] = 1;
        return limit;
    }
    // ops executed by kernels that only know fp32 NCHW pin their tensors to it
    void pin_fp32(const BlobOp &op) {
        for (uint32_t j = 0; j < op.n_src; ++j) cand[op.src[j].tensor] = 0;
        cand[op.dst] = 0;
    }
    Step &push(StepKind kind, size_t i);
    Step &conv_step(size_t i, size_t ci, const KOrder &ko, const Dims &in, const Dims &out);
    void choose(Step &st, int need);

    int init(int H, int W, size_t ws_bytes);                       // 1
    int walk_ops();                                                // 2
    bool front_fits(size_t i, const StemArgs &a, const Dims &out) const;
    int stem_op(size_t &i, const Dims &out);
    int conv_op(size_t &i, const Dims &in, const Dims &out);
    bool can_commute_upsample(size_t i, const Dims &in, const Dims &out) const;
    void commuted_upsample(size_t &i, const Dims &in, const Dims &out);
    void head_op(size_t i, const Dims &in);
    void plain_op(size_t i, const Dims &in, const Dims &out);
    void settle_formats();                                         // 3
    int pick_kernels();                                            // 4
    int pick_fp32_kernel(Step &st);
    void pair_and_share();                                         // 5
    void share_add(size_t k, size_t &w);
    Step pair_step(size_t k) const;
    void fold(FoldForm form);                                      // 6
    void fold_into(Step &sl, const Step &sr, FoldForm form);
};

// ---- 1. dims and workspace layout; the options and the bookkeeping the other passes read
int Sched::init(int H, int W, size_t ws_bytes) {
    size_t ws_need = 0;
    int rc = layout(p, B, H, W, d, off, ws_need, &share_off);
    if (rc) return rc;
    if (ws_bytes < ws_need) return fail(PF_EWORKSPACE, "workspace %zu B < required %zu B", ws_bytes, ws_need);
    input = p->net.ops[0].src[0].tensor;

    // option "profile_tag_ops" (per plan, or process-wide for tools that switch it on late): per-op labels in pf_profile_* records
    tags = (p->opt.profile_tag_ops != 0 || g_plan_opt.profile_tag_ops != 0) && prof_enabled();
    fuse = p->opt.fuse_pool != 0;      // option "fuse_pool"
    // pf_set_option("fuse_upsample", 0/1); at B=4: transUp.3 + conv1x1_up.3 144 us fused vs 233 us as two passes
    fuse_up = p->opt.fuse_upsample != 0;   // option "fuse_upsample"
    Bt = p->opt.table_batch > 0 ? p->opt.table_batch : B;
    // range guard of the two-term operand split (conv_mfma.h): producers of tensors a split kernel may read raise
    // PF_STATUS_RANGE in the live status word and report their max |v| to their op's slot; the forward ends with range_finalize
    // (PF_STATUS_RANGE_LOW, published status word, sticky word, everything live cleared for the next forward).  fp32-only plans
    // clamp nothing and check nothing
    st_words = reinterpret_cast<unsigned *>(ws);
    status_all = (p->opt.split_f16 && p->opt.range_guard) ? st_words + kLiveWord : nullptr;

    const size_t nT = p->net.tensors.size();
    fmt.assign(nT, 0);
    cand.assign(nT, 1);
    written.resize(nT);
    for (size_t t = 0; t < nT; ++t) written[t].assign(p->net.tensors[t].channels + 8, 0);
    s4_allowed = p->opt.packed_acts && p->opt.split_f16 && force_allows_s4();

    steps.clear();
    steps.reserve(2 * p->net.ops.size());   // at most two steps per op: no reallocation while a Step & is held
    return PF_OK;
}

Step &Sched::push(StepKind kind, size_t i) {
    Step &st = steps.emplace_back();
    memset(&st, 0, sizeof(st));
    st.kind = kind; st.op = (int)i;
    const BlobOp &o = p->net.ops[i];
    const Dims out = o.kind == OP_HEAD ? d[o.src[0].tensor] : d[o.dst];
    if (tags) snprintf(st.tag, sizeof(st.tag), "%02zu %s %u->%u %dx%d", i, p->net.tensors[o.dst].name, o.cin, o.cout, out.h, out.w);
    return st;
}

// a step of op i running convolution ci over the ranges ko
Step &Sched::conv_step(size_t i, size_t ci, const KOrder &ko, const Dims &in, const Dims &out) {
    Step &st = push(S_CONV, i);
    const BlobOp &o = p->net.ops[ci];
    ConvArgs &a = st.u.c;
    st.ci = (int)ci; st.dst_t = o.dst;
    set_sources(a, ko, [this](uint32_t t) { return tref(t); });
    for (int j = 0; j < ko.n; ++j) st.src_t[j] = ko.r[j].tensor;
    a.bias = p->dev_weights + p->conv[ci].bias_off;
    a.dst = tptr(o.dst);
    a.dst_ctotal = (int)p->net.tensors[o.dst].channels; a.dst_choff = (int)o.dst_choff;
    a.Cin = (int)o.cin; a.Cout = (int)o.cout;
    a.Hin = in.h; a.Win = in.w; a.Hout = out.h; a.Wout = out.w;
    a.relu = (int)o.relu;
    a.zero_page = p->dev_weights;   // first 64 floats of the weight arena are zeros
    a.ntiles = ((int)o.cout + 15) / 16;
    a.acc_scale = 1.0f;
    a.status = status_of(o.dst); a.range_slot = slot_of(ci, o.dst);
    return st;
}

// its kernels (conv_select.cpp: decide_conv) and what it can read / write as S4
void Sched::choose(Step &st, int need) {
    const BlobOp &o = p->net.ops[st.ci];
    const ConvPlan &cp = p->conv[st.ci];
    const ConvArgs &a = st.u.c;
    const bool generic = (a.Win & 3) != 0;
    st.dec = decide_conv({(int)o.k, (int)o.stride, a.Cin, a.Cout, a.Hout, a.Wout, Bt, need, generic, cp.split_off != 0, cp.s4_off != 0,
                          p->opt.use_tuned_table != 0, p->opt.split_f16 != 0, false, cp.s4_rounds, conv_force()});
    st.need = need; st.sb = a.src_begin; st.se = a.src_end;
    const bool res_fits = !a.res || (size_t)st.dec.s4.NT * 16 * res_chan_stride(res_extent(8, a.res_sh), res_extent(32, a.res_sw)) * sizeof(float) <= 60 * 1024;
    st.can_read = s4_allowed && o.kind == OP_CONV && st.dec.wants_s4 && res_fits && ((a.src_begin == 0 && a.src_end == a.n_src) || cp.s4_pad);
    st.can_write_s4 = s4_allowed && !generic && (a.dst_choff & 1) == 0;
    st.can_write = st.can_write_s4 && (st.dec.ch.is(CONV_DMA) || st.dec.ch.is(CONV_SPLIT));
    st.u.c.dst_limit = claim(st.dst_t, a.dst_choff, a.dst_choff + a.Cout);
}

// ---- 2. one walk over the ops: fusions (front, pool, commuted upsample) and each convolution's choice
int Sched::walk_ops() {
    cand[input] = 0;
    for (size_t i = 0; i < p->net.ops.size(); ++i) {
        const BlobOp &o = p->net.ops[i];
        const Dims in = d[o.src[0].tensor];
        const Dims out = o.kind == OP_HEAD ? in : d[o.dst];
        int rc = PF_OK;
        if (o.kind == OP_STEM && stem) rc = stem_op(i, out);
        else if (o.kind == OP_STEM || o.kind == OP_CONV) rc = conv_op(i, in, out);
        else if (o.kind == OP_UPSAMPLE && can_commute_upsample(i, in, out)) commuted_upsample(i, in, out);
        else if (o.kind == OP_HEAD) head_op(i, in);
        else plain_op(i, in, out);   // OP_POOL, OP_UPSAMPLE
        if (rc) return rc;
    }
    return PF_OK;
}

// stem -> [3x3 s1 16 -> 24] -> [3x3 s2 24 -> <= 32] with single readers: the two convs run as conv_front.hip on the
// packed-pair stem output; the tensor between them is never stored
bool Sched::front_fits(size_t i, const StemArgs &a, const Dims &out) const {
    if (!(s4_allowed && p->opt.fuse_front && i + 2 < p->net.ops.size())) return false;
    const BlobOp &o = p->net.ops[i], &n1 = p->net.ops[i + 1], &n2 = p->net.ops[i + 2];
    return n1.kind == OP_CONV && n1.k == 3 && n1.stride == 1 && n1.n_src == 1 && n1.src[0].tensor == o.dst && n1.src[0].choff == 0 &&
           n1.src[0].ch == p->net.tensors[o.dst].channels && n1.dst_choff == 0 && n1.cout == p->net.tensors[n1.dst].channels &&
           p->readers[o.dst] == 1 && p->readers[n1.dst] == 1 && n1.relu && p->conv[i + 1].s4_off && p->conv[i + 1].s4_rounds == 2 &&
           n2.kind == OP_CONV && n2.k == 3 && n2.stride == 2 && n2.n_src == 1 && n2.src[0].tensor == n1.dst && n2.src[0].choff == 0 &&
           n2.src[0].ch == n1.cout && p->conv[i + 2].front_off && (n2.dst_choff & 3) == 0 &&
           conv_front_supports((int)o.cout, (int)n1.cout, (int)n2.cout, out.h, out.w, (int)p->net.tensors[n2.dst].channels) && stem_family(a) == STEM_V4 && !conv_forced();
}

// the fused one-hot stem of pf_bg_forward, alone or with the front end behind it (then i ends on the front end's second conv)
int Sched::stem_op(size_t &i, const Dims &out) {
    const BlobOp &o = p->net.ops[i];
    StemArgs a = *stem;
    a.w = p->dev_weights + p->conv[i].raw_off; a.wdep = p->dev_weights + p->conv[i].dep_off;
    a.woh = p->conv[i].oh_off ? p->dev_weights + p->conv[i].oh_off : nullptr; a.bias = p->dev_weights + p->conv[i].bias_off;
    a.status = status_of(o.dst); a.range_slot = slot_of(i, o.dst);
    a.lut = p->dev_lut; a.dst = tptr(o.dst); a.Hout = out.h; a.Wout = out.w;
    if (!front_fits(i, a, out)) {
        if (o.cout != 16 || o.k != 3 || o.stride != 2 || o.dst_choff != 0 ||
            p->net.tensors[o.dst].channels != 16 || (uint32_t)(a.T * (a.n_cls + 1)) != o.cin)
            return fail(PF_EUNSUPPORTED, "fused stem expects a 3x3/s2 conv %d->16, got %u->%u k%u s%u",
                        a.T * (a.n_cls + 1), o.cin, o.cout, o.k, o.stride);
        push(S_STEM, i).u.sf.stem = a;
        pin_fp32(o);
        return PF_OK;
    }
    const BlobOp &n1 = p->net.ops[i + 1], &n2 = p->net.ops[i + 2];
    const Dims o2 = d[n2.dst];   // (the front end's output)
    cand[o.dst] = 0; cand[n1.dst] = 0;   // (not subject to the format decision: the stem output is packed, the middle tensor never exists)
    Step &st = push(S_STEM_FRONT, i);
    st.u.sf.stem = a; st.u.sf.stem.dst_fmt = 1;
    FrontArgs &f = st.u.sf.front;
    f.x = tptr(o.dst);
    f.w1 = p->dev_weights + p->conv[i + 1].s4_off; f.w2 = p->dev_weights + p->conv[i + 2].front_off;
    f.bias1 = p->dev_weights + p->conv[i + 1].bias_off; f.bias2 = p->dev_weights + p->conv[i + 2].bias_off;
    f.scale1 = p->conv[i + 1].split_acc_scale; f.scale2 = p->conv[i + 2].split_acc_scale;
    f.dst = tptr(n2.dst);
    f.dst_ctotal = (int)p->net.tensors[n2.dst].channels; f.dst_c4 = (f.dst_ctotal + 3) / 4; f.dst_choff = (int)n2.dst_choff;
    f.dst_limit = claim(n2.dst, f.dst_choff, f.dst_choff + (int)n2.cout);
    f.H1 = out.h; f.W1 = out.w; f.H2 = o2.h; f.W2 = o2.w;
    f.C1 = (int)n1.cout; f.C2 = (int)n2.cout; f.relu1 = (int)n1.relu; f.relu2 = (int)n2.relu;
    f.status = status_all;
    f.range_slot_mid = slot_of(i + 1, n1.dst); f.range_slot = slot_of(i + 2, n2.dst);
    st.dst_t = n2.dst; st.can_write = st.can_write_s4 = true;
    if (tags)
        snprintf(st.u.sf.front_tag, sizeof(st.u.sf.front_tag), "%02zu+%02zu %s+%s %u->%u->%u %dx%d", i + 1, i + 2, p->net.tensors[n1.dst].name,
                 p->net.tensors[n2.dst].name, o.cout, n1.cout, n2.cout, o2.h, o2.w);
    i += 2;
    return PF_OK;
}

// a convolution (a stem without the fused kernel's inputs is one), with the 2x2 average pool behind it in its epilogue where that fits
int Sched::conv_op(size_t &i, const Dims &in, const Dims &out) {
    const BlobOp &o = p->net.ops[i];
    if (o.src[0].tensor == input && !dense_x)
        return fail(PF_EINVAL, "network input is consumed by a generic conv: use pf_hardnet_forward_dense");
    // a caller-provided dense input has no producer kernel that could have checked its range
    // (its maximum goes to the last slot of the block: the input has no op of its own)
    if (o.src[0].tensor == input && status_all) {
        PlainArgs &x = push(S_RANGE_CHECK, i).u.x;
        x.src = dense_x; x.n = (size_t)B * p->net.tensors[input].channels * in.h * in.w;
        x.status = status_all; x.slot = st_words + kSlot0 + kMaxSlots - 1;
    }
    // conv + AvgPool2d(2,2): pool in the conv epilogue, the full-resolution tensor is never written
    const BlobOp *pool = nullptr;
    if (fuse && i + 1 < p->net.ops.size() && p->net.ops[i + 1].kind == OP_POOL && o.stride == 1 && o.k == 1 && (in.w & 3) == 0 &&
        p->net.ops[i + 1].src[0].tensor == o.dst && o.dst_choff == 0 && o.cout == p->net.tensors[o.dst].channels &&
        p->readers[o.dst] == 1 && out.h >= 2 && out.w >= 2)
        pool = &p->net.ops[i + 1];
    Step &st = conv_step(i, i, order_plain(o.src, (int)o.n_src), in, out);
    if (pool) {
        ConvArgs &a = st.u.c;
        a.pool = 1; a.dst = tptr(pool->dst); a.dst_ctotal = (int)p->net.tensors[pool->dst].channels;
        st.dst_t = pool->dst;
        a.status = status_of(pool->dst); a.range_slot = slot_of(i, pool->dst);
        ++i;   // the pool op is done
    }
    choose(st, pool ? 2 : 0);
    return PF_OK;
}

bool Sched::can_commute_upsample(size_t i, const Dims &in, const Dims &out) const {
    if (!fuse || !fuse_up || i + 1 >= p->net.ops.size()) return false;
    const BlobOp &o = p->net.ops[i], &n = p->net.ops[i + 1];
    return n.kind == OP_CONV && n.k == 1 && n.stride == 1 && n.n_src == 2 && n.src[0].tensor == o.dst &&
           n.src[0].choff == 0 && n.src[0].ch == p->net.tensors[o.dst].channels && p->readers[o.dst] == 1 &&
           (in.w & 3) == 0 && (out.w & 3) == 0 && n.cout <= p->net.tensors[o.dst].channels &&
           2 * in.h <= out.h + 1 && 2 * in.w <= out.w + 1;   // >= ~2x upsampling: the residual window of a tile stays small
}

// TransitionUp + 1x1 conv over cat([up(x), skip])  ==  W_skip*skip + up(W_x*x)   (conv_epilogue.h): two steps under the upsample's op
void Sched::commuted_upsample(size_t &i, const Dims &in, const Dims &out) {
    const BlobOp &o = p->net.ops[i], &n = p->net.ops[i + 1];
    const Dims hi = out;   // = size of the skip tensor
    cand[o.dst] = 0;       // sampled as an fp32 residual by the other half
    auto tag_half = [&](Step &st, const char *half, int cin, const Dims &dd) {
        if (tags)
            snprintf(st.tag, sizeof(st.tag), "%02zu%c %s.%s %d->%u %dx%d", i + 1, half[0] == 'l' ? 'a' : 'b', p->net.tensors[n.dst].name,
                     half, cin, n.cout, dd.h, dd.w);
    };
    const KOrder kn = order_plain(n.src, (int)n.n_src);
    KOrder kx = kn;                                    // range 0: x at the low resolution
    kx.r[0].tensor = o.src[0].tensor; kx.r[0].choff = (int)o.src[0].choff;
    Step &ls = conv_step(i, i + 1, kx, in, in);
    ConvArgs &lo = ls.u.c;
    lo.dst = tptr(o.dst);                              // scratch: the slot of the (never built) upsampled tensor
    ls.dst_t = o.dst;
    lo.dst_ctotal = (int)n.cout; lo.dst_choff = 0;
    lo.relu = 0; lo.no_bias = 1;
    lo.status = nullptr; lo.range_slot = nullptr;      // an fp32 residual of the other half, never a split operand
    lo.Cin = (int)n.src[0].ch;
    lo.src_end = 1;
    tag_half(ls, "lo", lo.Cin, in);
    choose(ls, 4);
    Step &hs = conv_step(i, i + 1, kn, hi, hi);
    ConvArgs &ha = hs.u.c;
    ha.Cin = (int)n.src[1].ch;
    ha.src_begin = 1; ha.src_end = 2;
    tag_half(hs, "hi", ha.Cin, hi);
    ha.res = tptr(o.dst); ha.res_ctotal = (int)n.cout;
    ha.Hres = in.h; ha.Wres = in.w;
    ha.res_sh = hi.h > 1 ? (float)(in.h - 1) / (float)(hi.h - 1) : 0.f;
    ha.res_sw = hi.w > 1 ? (float)(in.w - 1) / (float)(hi.w - 1) : 0.f;
    choose(hs, 4);
    ++i;   // the 1x1 conv is done
}

void Sched::head_op(size_t i, const Dims &in) {
    const BlobOp &o = p->net.ops[i];
    pin_fp32(o);
    Step &st = push(S_HEAD, i);
    HeadArgs &a = st.u.head.h;
    a.logits = tptr(o.src[0].tensor);
    a.out_seg = out_seg; a.out_logits = out_logits; a.out_is_i64 = out_seg_is_i64;
    a.B = B; a.C = (int)o.cin; a.Hin = in.h; a.Win = in.w; a.Hout = out_h; a.Wout = out_w;
    st.u.head.orig = out_orig; st.u.head.orig_bytes = (size_t)B * a.C * in.h * in.w * sizeof(float);
}

// a pool or an upsample as a launch of its own
void Sched::plain_op(size_t i, const Dims &in, const Dims &out) {
    const BlobOp &o = p->net.ops[i];
    pin_fp32(o);
    PlainArgs &x = push(o.kind == OP_POOL ? S_POOL : S_UPSAMPLE, i).u.x;
    x.src = tptr(o.src[0].tensor); x.dst = tptr(o.dst); x.planes = B * (int)o.cin;
    x.hin = in.h; x.win = in.w; x.hout = out.h; x.wout = out.w;
    x.status = status_of(o.dst); x.slot = slot_of(i, o.dst);
}

// ---- 3. formats, a fixpoint: a launch reads S4 only if ALL the ranges it accumulates are S4; a tensor stays S4 only while
//      all its readers do and all its writers can
void Sched::settle_formats() {
    if (!s4_allowed) std::fill(cand.begin(), cand.end(), 0);
    for (bool changed = true; changed;) {
        changed = false;
        for (const Step &r : steps) {
            if (r.kind != S_CONV && r.kind != S_STEM_FRONT) continue;
            bool all = r.can_read;
            for (int j = r.sb; j < r.se; ++j) all = all && cand[r.src_t[j]];
            if (!all)
                for (int j = r.sb; j < r.se; ++j)
                    if (cand[r.src_t[j]]) { cand[r.src_t[j]] = 0; changed = true; }
            if (!(r.can_write || (all && r.can_write_s4)) && cand[r.dst_t]) { cand[r.dst_t] = 0; changed = true; }
        }
    }
    // a tensor nobody reads as S4 (network outputs tapped by the caller) stays fp32
    const size_t nT = p->net.tensors.size();
    std::vector<uint8_t> read_s4(nT, 0);
    for (const Step &r : steps)
        if (r.kind == S_CONV)
            for (int j = r.sb; j < r.se; ++j) read_s4[r.src_t[j]] = 1;
    for (size_t t = 0; t < nT; ++t) fmt[t] = cand[t] && read_s4[t];
}

// ---- 4. each convolution's kernel: S4 sources, or its fp32-source kernel where that one has a kernel for the launch, else conv_dma
int Sched::pick_kernels() {
    for (Step &st : steps) {
        if (st.kind == S_STEM_FRONT) {
            st.u.sf.front.dst_fmt = fmt[st.dst_t];
            fmt[p->net.ops[st.op].dst] = 1;            // pf_hardnet_tensor_read unpacks the stem output
            fmt[p->net.ops[st.op + 1].dst] = 0xFF;     // ... and refuses the tensor between the two convs: it is never stored
        }
        if (st.kind != S_CONV) continue;
        const BlobOp &o = p->net.ops[st.ci];
        const ConvPlan &cp = p->conv[st.ci];
        ConvArgs &a = st.u.c;
        a.dst_fmt = fmt[st.dst_t]; a.dst_c4 = (a.dst_ctotal + 3) / 4;
        bool s4 = st.can_read;
        for (int j = st.sb; j < st.se; ++j) s4 = s4 && fmt[st.src_t[j]];
        if (s4) {
            a.src_fmt = 1; a.acc_scale = cp.split_acc_scale;
            a.wpk = p->dev_weights + cp.s4_off; a.nchunks = cp.s4_rounds;
            set_s4_entries(a, (int)o.k, cp.s4_pad);
            st.kind = S_CONV_S4; continue;
        }
        if (int rc = pick_fp32_kernel(st)) return rc;
    }
    return PF_OK;
}

// a convolution over fp32 NCHW sources: the generic kernel on a width % 4 != 0, else dec.ch as far as that family has the shape built
int Sched::pick_fp32_kernel(Step &st) {
    const BlobOp &o = p->net.ops[st.ci];
    const ConvPlan &cp = p->conv[st.ci];
    ConvArgs &a = st.u.c;
    if ((a.Win & 3) != 0) {
        if (st.need) return fail(PF_EUNSUPPORTED, "fused conv on a width that is not a multiple of 4");
        a.wpk = p->dev_weights + cp.wpk_off; a.nchunks = cp.tiling.nchunks;
        st.kind = S_CONV_GENERIC; return PF_OK;
    }
    auto use = [&](size_t wpk_off, int nchunks, int kc) {   // a packing of the weights in chunks of kc input channels
        a.wpk = p->dev_weights + wpk_off;
        a.nchunks = nchunks;
        set_chunks(a, kc);
    };
    ConvChoice &ch = st.dec.ch;
    if (ch.is(CONV_SPLIT)) {
        use(cp.split_off, cp.split_chunks, o.k == 1 ? 32 : 8);
        a.acc_scale = cp.split_acc_scale;
        st.kind = o.k == 1 ? S_CONV_SPLIT1 : S_CONV_SPLIT;
        if (o.k == 1 ? conv_split1_supported(a, ch.split_nt()) : conv_split_supported(a)) return PF_OK;
        ch = ConvChoice::dma();
    }
    if (ch.is(CONV_WAVE)) {
        use(cp.wave_off, cp.wave_chunks, wave_kc((int)o.k));
        ch = ConvChoice::wave(ch.wave_mh(), ch.wave_nt() < a.ntiles ? ch.wave_nt() : a.ntiles, ch.wave_wk());
        st.kind = S_CONV_WAVE;
        if (conv_wave_supported(a, (int)o.k, ch.wave_mh(), ch.wave_nt(), ch.wave_wk())) return PF_OK;
        ch = ConvChoice::dma();   // shape not built: conv_dma with its cost model
    }
    use(cp.tiled_off, cp.tiled_chunks, dma_kc((int)o.k, (int)o.stride));
    st.kind = S_CONV_DMA;
    // the trailing rem_count output channels of a big image go to the vector ALU instead of an MFMA tile
    // (conv_dma WM=4 shapes only, forced or cost-model-chosen)
    int wm, nt;
    if (p->opt.valu_remainder && cp.rem_off && !st.need && !a.dst_fmt && a.src_begin == 0 && a.src_end == a.n_src && (ch.dma_wm() == 0 || ch.dma_wm() == 4)) {
        ConvArgs r = a;
        r.rem = cp.rem_count;
        r.wrem = p->dev_weights + cp.rem_off;
        r.ntiles = ((int)o.cout - r.rem) / 16;
        if (conv_dma_supported(r, (int)o.k, (int)o.stride, B, 4, ch.dma_wm() == 4 && ch.dma_nt() > 0 ? ch.dma_nt() : 0, p->opt.table_batch, &wm, &nt)) {
            a = r;
            ch = ConvChoice::dma(wm, nt);
            return PF_OK;
        }
    }
    conv_dma_supported(a, (int)o.k, (int)o.stride, B, ch.dma_wm(), ch.dma_nt(), p->opt.table_batch, &wm, &nt);   // (no kernel: the launcher says so)
    ch = ConvChoice::dma(wm, nt);
    return PF_OK;
}

// ---- 5. an odd HarDBlock layer inside its consumer (conv_pair.hip): two adjacent steps P = op i, C = op i + 1 that both read
//      and write packed pairs become one; or (conv_s4.hip share / add) stay two launches that read their common source S once: P's
//      launch also sums C's rows over S, C's launch runs over its other ranges and adds them
void Sched::pair_and_share() {
    size_t w = 0;
    for (size_t k = 0; k < steps.size(); ++k, ++w) {
        const size_t i = (size_t)steps[k].op;
        // (reading S4 implies a width % 4 == 0 and no forced kernel but conv_s4)
        const bool adjacent = k + 1 < steps.size() && steps[k].kind == S_CONV_S4 && steps[k + 1].kind == S_CONV_S4 && steps[k + 1].op == (int)i + 1 &&
                              is_conv_pair(p->net, i) && steps[k].u.c.dst_fmt && steps[k + 1].u.c.dst_fmt;
        const bool pair = p->opt.fuse_pairs && adjacent && p->conv[i + 1].pair_c_off;
        const BlobOp &o = p->net.ops[i];
        if (pair && pair_wanted((int)o.cin, (int)o.cout, (int)p->net.ops[i + 1].cin, (int)p->net.ops[i + 1].cout, d[o.dst].h, d[o.dst].w, Bt,
                                p->opt.fuse_pairs)) {
            steps[w] = pair_step(k);
            ++k;
        // share / add: 8 x 32 tiles without a K split for both launches, packings made at plan creation
        } else if (adjacent && p->opt.share_s && p->conv[i + 1].share_a_off && share_off != (size_t)-1 && steps[k].dec.s4_tile == S4_8x32 && steps[k + 1].dec.s4_tile == S4_8x32 &&
                   share_wanted((int)o.cin, (int)o.cout, (int)p->net.ops[i + 1].cin, (int)p->net.ops[i + 1].cout, d[o.dst].h, d[o.dst].w, Bt, p->opt.share_s)) {
            share_add(k, w);
            ++k;
        } else if (w != k) {
            steps[w] = steps[k];
        }
    }
    steps.resize(w);
}

// steps k, k + 1 (P, C) as the share and the add launch, stored at w, w + 1 (w ends on the second)
void Sched::share_add(size_t k, size_t &w) {
    const size_t i = (size_t)steps[k].op;
    const BlobOp &o = p->net.ops[i];
    const ConvPlan &cc = p->conv[i + 1];
    Step sa = steps[k], sb = steps[k + 1];
    float *const sums = reinterpret_cast<float *>((char *)ws + share_off);
    ConvArgs &a = sa.u.c, &c = sb.u.c;
    sa.kind = S_CONV_S4_SHARE;
    a.wpk = p->dev_weights + cc.share_a_off; a.ntiles = cc.share_a_tiles;
    a.share = sums; a.share_off = share_row0((int)o.cout); a.share_cout = c.Cout; a.share_scale = cc.split_acc_scale;
    sa.dec.s4_nt = cc.share_a_tiles <= 3 ? cc.share_a_tiles : 2;
    // the consumer without its second range S
    sb.kind = S_CONV_S4_ADD;
    set_sources(c, order_add(p->net.ops[i + 1].src, (int)p->net.ops[i + 1].n_src), [this](uint32_t t) { return tref(t); });
    c.Cin = c.src_cstart[c.n_src];
    c.wpk = p->dev_weights + cc.share_b_off; c.nchunks = cc.share_b_rounds;
    set_s4_entries(c, 3, 0);
    c.share = sums; c.share_cout = c.Cout;
    steps[w] = sa;
    steps[++w] = sb;
}

// steps k, k + 1 (P, C) as one conv_pair launch: the consumer's S4 launch (pa.c) with its sources in the pair's K order [S, others.., P]
Step Sched::pair_step(size_t k) const {
    const size_t i = (size_t)steps[k].op;
    const BlobOp &o = p->net.ops[i], &C = p->net.ops[i + 1];
    Step st = steps[k + 1];
    st.kind = S_PAIR; st.op = (int)i;
    if (tags)
        snprintf(st.tag, sizeof(st.tag), "%02zu+%02zu %s+%s %u->%u->%u %dx%d", i, i + 1, p->net.tensors[o.dst].name, p->net.tensors[C.dst].name, o.cin,
                 o.cout, C.cout, d[o.dst].h, d[o.dst].w);
    PairArgs &pa = st.u.pair;
    ConvArgs &a = pa.c;
    const int n = (int)C.n_src;
    set_sources(a, order_pair(C.src, n), [this](uint32_t t) { return tref(t); });
    a.wpk = p->dev_weights + p->conv[i + 1].pair_c_off; a.nchunks = p->conv[i + 1].pair_rounds;
    set_s4_entries(a, 3, 1);
    pa.p_wpk = p->dev_weights + p->conv[i + 1].pair_two_off; pa.p_w9 = p->dev_weights + p->conv[i + 1].pair_nine_off;
    pa.p_bias = p->dev_weights + p->conv[i].bias_off; pa.p_acc_scale = p->conv[i].split_acc_scale;
    pa.p_dst = tptr(o.dst); pa.p_dst_c4 = ((int)p->net.tensors[o.dst].channels + 3) / 4;
    pa.p_dst_choff = (int)o.dst_choff; pa.p_dst_limit = steps[k].u.c.dst_limit;
    pa.p_cout = (int)o.cout; pa.p_cin = (int)o.cin; pa.p_ntiles = ((int)o.cout + 15) / 16; pa.p_relu = (int)o.relu;
    pa.p_range_slot = slot_of(i, o.dst);
    pa.rounds_s = a.src_ent0[1] / 2; pa.round_d = a.src_ent0[n - 1] / 2;
    pa.merged = p->conv[i + 1].pair_merged && p->opt.fuse_pairs != 3;
    return st;
}

// ---- 6. the folds of conv_s4.hip, one form per call: a 3x3 conv L and the 1x1 conv R that reads its slice last (is_conv_fold) as
//      ONE launch.  Two adjacent plain conv_s4 steps - not part of a pair or a share / add step, whose kinds differ -, L on
//      <2, 32, 8, 1> or, the wide forms, <3, 32, 8, 1> into packed pairs; R's step goes away.  (up: R's step is the low-resolution half of
//      the commuted upsample + 1x1 conv, made under the upsample's op; the other half stays as it is)
void Sched::fold(FoldForm form) {
    const FoldDesc &f = kFolds[form];
    const int mode = p->opt.*f.option;
    for (size_t k = 0; mode && p->fold[form].dev && k + 1 < steps.size(); ++k) {
        Step &sl = steps[k];
        const Step &sr = steps[k + 1];
        const size_t i = (size_t)sl.op;
        if (sl.kind != S_CONV_S4 || sr.kind != S_CONV_S4 || sl.ci != (int)i || sr.op != (int)i + 1 || sr.ci != (int)(i + f.r_at())) continue;
        if (!p->conv[i].fold_off[form] || !is_conv_fold(p->net, i, form)) continue;
        const BlobOp &L = p->net.ops[i], &R = p->net.ops[i + f.r_at()];
        const ConvArgs &a = sl.u.c, &r = sr.u.c;
        const S4Shape &sh = sl.dec.s4;
        if (sh.NT != f.l_tiles || sh.TW != 32 || sh.TH != 8 || sh.KS != 1 || !a.dst_fmt || r.res || a.Hout != r.Hout || a.Wout != r.Wout) continue;
        // tail: R without fused stages into fp32, nothing of it range-checked.  down: R with its pool fused and nothing else, into
        // packed pairs or fp32.  lo: the first range of R alone, without bias or ReLU, into fp32
        if (f.up ? (!r.no_bias || r.relu || r.src_begin != 0 || r.src_end != 1 || r.dst_fmt || r.status || r.pool)
                 : r.no_bias || (form == FOLD_TAIL ? (r.dst_fmt || r.status || r.pool) : (!r.pool || !r.relu)))
            continue;
        if (!f.wanted((int)L.cin, (int)L.cout, (int)R.cout, a.Hout, a.Wout, Bt, mode)) continue;
        fold_into(sl, sr, form);
        steps.erase(steps.begin() + (long)k + 1);
    }
}

// L's step sl takes R's operands and destination from R's step sr
void Sched::fold_into(Step &sl, const Step &sr, FoldForm form) {
    const FoldDesc &f = kFolds[form];
    const size_t i = (size_t)sl.op;
    const BlobOp &L = p->net.ops[i], &R = p->net.ops[i + f.r_at()];
    ConvArgs &a = sl.u.c;
    const ConvArgs &r = sr.u.c;
    const KOrder ko = order_tail(p->net.ops[i + 1].src[0], (int)L.dst_choff, (int)L.cout);
    a.fold_w = p->fold[form].dev + p->conv[i].fold_off[form];
    a.fold_bias = f.up ? a.zero_page : r.bias; a.fold_scale = r.acc_scale; a.fold_cout = r.Cout;
    a.fold_src = a.dst; a.fold_c4 = a.dst_c4; a.fold_g0 = ko.r[0].choff / 4; a.fold_gn = ko.r[0].ch / 4;
    if (form == FOLD_TAIL || form == FOLD_LO) {
        a.tail_dst = r.dst; a.tail_ctotal = r.dst_ctotal; a.tail_choff = r.dst_choff;
        sl.kind = form == FOLD_TAIL ? S_CONV_S4_TAIL : S_CONV_S4_LO;
        // lo: the slice is stored as ever unless the upsample is the only op that reads it
        bool read_elsewhere = false;
        for (size_t j = 0; j < p->net.ops.size(); ++j)
            for (uint32_t q = 0; q < p->net.ops[j].n_src && j != i + 1; ++q) {
                const BlobSrc &os = p->net.ops[j].src[q];
                read_elsewhere = read_elsewhere || (os.tensor == L.dst && os.choff < L.dst_choff + L.cout && os.choff + os.ch > L.dst_choff);
            }
        if (form == FOLD_TAIL || !read_elsewhere) {
            fmt[L.dst] = 0xFE;   // pf_hardnet_tensor_read refuses the tensor: its last slice is never stored
            if (form == FOLD_LO) a.dst = nullptr;
        }
    } else {   // L's slice is stored as ever
        a.down_dst = r.dst; a.down_c4 = r.dst_c4; a.down_choff = r.dst_choff; a.down_limit = r.dst_limit;
        a.down_fmt = r.dst_fmt; a.down_ctotal = r.dst_ctotal;
        a.down_status = r.status; a.down_slot = r.range_slot;
        sl.kind = S_CONV_S4_DOWN;
    }
    if (tags)
        snprintf(sl.tag, sizeof(sl.tag), "%02zu+%02zu %s+%s %u->%u->%u %dx%d", i, i + f.r_at(), p->net.tensors[L.dst].name, p->net.tensors[R.dst].name, L.cin,
                 L.cout, R.cout, a.Hout, a.Wout);
}

}  // namespace

int build_schedule(const pf_plan *p, const StemArgs *stem, const float *dense_x, int B, int H, int W, int out_h, int out_w,
                   void *out_seg, int out_seg_is_i64, float *out_logits, float *out_orig, void *ws, size_t ws_bytes,
                   std::vector<Step> &steps, std::vector<uint8_t> &fmt) {
    Sched s{p, stem, dense_x, B, out_h, out_w, out_seg, out_seg_is_i64, out_logits, out_orig, ws, steps, fmt};
    if (int rc = s.init(H, W, ws_bytes)) return rc;
    if (int rc = s.walk_ops()) return rc;
    s.settle_formats();
    if (int rc = s.pick_kernels()) return rc;
    s.pair_and_share();
    for (int form = 0; form < kFoldForms; ++form) s.fold((FoldForm)form);
    return PF_OK;
}

}  // namespace pf

using namespace pf;

// ---- pf_debug_hardnet_schedule (include/pfhip.h documents the columns)
// FNV-1a over a step's labels and the argument struct its launcher is handed (zero-filled at push and copied whole, so made-up
// fixed bases give the same bytes every time)
static uint64_t step_arg_hash(const Step &st) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void *q, size_t n) {
        for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)q)[i]) * 1099511628211ull;
    };
    mix(st.tag, sizeof(st.tag));
    if (is_conv_step(st.kind)) mix(&st.u.c, sizeof(st.u.c));
    else if (st.kind == S_PAIR) mix(&st.u.pair, sizeof(st.u.pair));
    else if (st.kind == S_STEM) mix(&st.u.sf.stem, sizeof(st.u.sf.stem));
    else if (st.kind == S_STEM_FRONT) mix(&st.u.sf, sizeof(st.u.sf));
    else if (st.kind == S_HEAD) mix(&st.u.head, sizeof(st.u.head));
    else mix(&st.u.x, sizeof(st.u.x));
    return h;
}

extern "C" int pf_debug_hardnet_schedule(const void *blob, size_t bytes, int in_ch, int n_cls, int B, int H, int W, int out_h, int out_w,
                                         int stem_T, int table_batch, unsigned char *formats, int cap_formats, int *n_formats,
                                         long long *steps, int cap_steps, int *n_steps) {
    if (!n_formats || !n_steps || (cap_formats > 0 && !formats) || (cap_steps > 0 && !steps) || B <= 0 || H <= 0 || W <= 0 || stem_T < 0)
        return fail(PF_EINVAL, "pf_debug_hardnet_schedule: bad argument");
    pf_plan p;
    std::vector<float> host;
    size_t n_floats = 0;
    if (int rc = debug_plan("pf_debug_hardnet_schedule", blob, bytes, in_ch, n_cls, &n_floats, p, host)) return rc;
    p.opt.table_batch = table_batch > 0 ? table_batch : 0;   // (per plan only: pf_hardnet_plan_set_option)
    // made-up addresses, far apart and fixed: the schedule computes with them and reads nothing through them
    char *const fake = (char *)(1ull << 44);
    auto base = [&](int n) { return fake + ((unsigned long long)n << 36); };
    p.dev_weights = (float *)base(0);
    p.dev_lut = (uint8_t *)base(1);
    for (int f = 0; f < kFoldForms; ++f)
        if (!p.fold[f].host.empty()) p.fold[f].dev = (float *)base(2 + f);
    std::vector<Dims> d;
    std::vector<size_t> off;
    size_t ws_bytes = 0;
    if (int rc = layout(&p, B, H, W, d, off, ws_bytes)) return rc;
    StemArgs stem;
    memset(&stem, 0, sizeof(stem));
    if (stem_T > 0) {   // as pf_bg_forward fills it
        if (p.net.ops.empty() || p.net.ops[0].kind != OP_STEM) return fail(PF_EUNSUPPORTED, "pf_debug_hardnet_schedule: plan does not start with a fused stem");
        stem.seg = base(10); stem.depth = (const float *)base(11); stem.mask = (const uint8_t *)base(12);
        stem.depth_mean = 20.f; stem.depth_std = 15.f; stem.min_depth = 0.1f; stem.max_depth = 200.f;
        stem.B = B; stem.T = stem_T; stem.n_cls = (int)p.net.hdr.n_cls; stem.H = H; stem.W = W;
    }
    std::vector<Step> sched;
    std::vector<uint8_t> fmt;
    if (int rc = build_schedule(&p, stem_T > 0 ? &stem : nullptr, stem_T > 0 ? nullptr : (const float *)base(9), B, H, W, out_h, out_w, base(13), 0,
                                (float *)base(14), (float *)base(15), base(8), ws_bytes, sched, fmt))
        return rc;
    *n_formats = (int)fmt.size();
    for (size_t t = 0; t < fmt.size() && (int)t < cap_formats; ++t) formats[t] = fmt[t];
    *n_steps = (int)sched.size();
    for (size_t k = 0; k < sched.size() && (int)k < cap_steps; ++k) {
        const Step &st = sched[k];
        const bool conv = is_conv_step(st.kind), s4 = st.kind >= S_CONV_S4 && st.kind <= S_CONV_S4_LO;
        const ConvArgs *a = conv ? &st.u.c : st.kind == S_PAIR ? &st.u.pair.c : nullptr;
        long long row[30] = {st.kind, st.op, a ? st.ci : -1};
        if (st.kind == S_CONV_S4_SHARE || st.kind == S_CONV_S4_ADD) {   // (the launchers clamp the request to 1 .. min(ntiles, 3))
            row[3] = std::max(1, std::min(std::min(st.dec.s4_nt, a->ntiles), 3)); row[4] = 32; row[5] = 8; row[6] = 1;
        } else if (s4) {
            row[3] = st.dec.s4.NT; row[4] = st.dec.s4.TW; row[5] = st.dec.s4.TH; row[6] = st.dec.s4.KS;
        } else if (conv) {
            row[7] = st.dec.ch.kind; row[8] = st.dec.ch.p0; row[9] = st.dec.ch.p1; row[10] = st.dec.ch.p2;
        }
        row[13] = a || st.kind == S_STEM_FRONT ? st.dst_t : p.net.ops[st.op].dst;
        if (st.kind == S_STEM_FRONT) row[12] = st.u.sf.front.dst_fmt;
        for (int j = 0; j < kConvMaxSrc; ++j) row[25 + j] = -1;
        if (a) {
            row[11] = a->src_fmt; row[12] = a->dst_fmt;
            row[14] = a->pool; row[15] = a->res != nullptr; row[16] = a->no_bias; row[17] = a->dst == nullptr;
            row[18] = a->ntiles; row[19] = a->nchunks; row[20] = a->fold_cout; row[21] = a->share_cout; row[22] = a->down_fmt;
            row[23] = st.sb; row[24] = st.se;
            for (int j = 0; j < (int)p.net.ops[st.ci].n_src; ++j) row[25 + j] = st.src_t[j];
        }
        row[29] = (long long)step_arg_hash(st);
        std::copy(row, row + 30, steps + 30 * k);
    }
    return PF_OK;
}
