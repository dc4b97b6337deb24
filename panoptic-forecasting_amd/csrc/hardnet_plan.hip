// A forward of a plan (hardnet_plan.h; built by plan_create.hip) = build_schedule (the op table -> a flat list of launches,
// every fusion and kernel choice made on the host) + an enqueue loop over it.
//
// Replaces the module walk of reference hardnet.py:353-387 (hardnet.forward) and the glue of
// bg_model.py:61-71,91-102.  The op table comes from the blob (packing.py / hardnet_arch.py); nothing
// about FC-HarDNet-70 is hard-coded here, so single-op test networks use the same code.
#include <cstdlib>
#include <cstring>

#include "hardnet_plan.h"
#include "pf_prof.h"

using namespace pf;

namespace {

// ---- A forward = build_schedule (host code only: every launch with all its arguments, each naming exactly one kernel) + the
//      enqueue loop of run_net.  S_CONV: inside build_schedule only, a convolution whose kernel is picked once the formats are known
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

int build_schedule(const pf_plan *p, const StemArgs *stem, const float *dense_x, int B, int H, int W, int out_h, int out_w,
                   void *out_seg, int out_seg_is_i64, float *out_logits, float *out_orig, void *ws, size_t ws_bytes,
                   std::vector<Step> &steps, std::vector<uint8_t> &fmt) {
    // ---- 1. dims and workspace layout
    std::vector<Dims> d;
    std::vector<size_t> off;
    size_t ws_need = 0;
    size_t share_off = (size_t)-1;
    int rc = layout(p, B, H, W, d, off, ws_need, &share_off);
    if (rc) return rc;
    if (ws_bytes < ws_need) return fail(PF_EWORKSPACE, "workspace %zu B < required %zu B", ws_bytes, ws_need);
    const uint32_t input = p->net.ops[0].src[0].tensor;
    auto tptr = [&](uint32_t t) -> float * {
        return t == input ? const_cast<float *>(dense_x) : reinterpret_cast<float *>((char *)ws + off[t]);
    };
    auto tref = [&](uint32_t t) { return TensorRef{tptr(t), (int)p->net.tensors[t].channels}; };

    // option "profile_tag_ops" (per plan, or process-wide for tools that switch it on late): per-op labels in pf_profile_* records
    const bool tags = (p->opt.profile_tag_ops != 0 || g_plan_opt.profile_tag_ops != 0) && prof_enabled();
    const bool fuse = p->opt.fuse_pool != 0;      // option "fuse_pool"
    const int Bt = p->opt.table_batch > 0 ? p->opt.table_batch : B;   // the batch every kernel choice is made for (option "table_batch")
    // range guard of the two-term operand split (conv_mfma.h): producers of tensors a split kernel may read raise
    // PF_STATUS_RANGE in the live status word and report their max |v| to their op's slot; the forward ends with range_finalize
    // (PF_STATUS_RANGE_LOW, published status word, sticky word, everything live cleared for the next forward).  fp32-only plans
    // clamp nothing and check nothing
    unsigned *const st_words = reinterpret_cast<unsigned *>(ws);
    unsigned *const status_all = (p->opt.split_f16 && p->opt.range_guard) ? st_words + kLiveWord : nullptr;
    // the guard of a launch: only if what it stores can become an operand of a split kernel (the logits cannot)
    auto status_of = [&](uint32_t dst_t) -> unsigned * { return p->feeds_conv[dst_t] ? status_all : nullptr; };
    auto slot_of = [&](size_t op_i, uint32_t dst_t) -> unsigned * {
        return (status_all && p->feeds_conv[dst_t]) ? st_words + kSlot0 + op_i : nullptr;
    };

    // Tensor formats: a tensor is S4 iff every step that reads it reads all its inputs as S4 and every step that writes it can
    // write S4.  cand = still possible; written = channels of each tensor some earlier step stores (half-group bookkeeping)
    const size_t nT = p->net.tensors.size();
    fmt.assign(nT, 0);
    std::vector<uint8_t> cand(nT, 1);
    std::vector<std::vector<uint8_t>> written(nT);
    for (size_t t = 0; t < nT; ++t) written[t].assign(p->net.tensors[t].channels + 8, 0);
    const bool s4_allowed = p->opt.packed_acts && p->opt.split_f16 && force_allows_s4();
    // a step stores channels [lo, hi) of tensor t: returns its S4 dst_limit (zero-fill the tail of the last group unless its owner
    // wrote it already)
    auto claim = [&](uint32_t t, int lo, int hi) -> int {
        std::vector<uint8_t> &wr = written[t];
        if ((lo & 3) == 2 && !wr[lo - 2]) cand[t] = 0;   // would expose an unwritten half group to readers of this range
        const int limit = ((hi & 3) != 0 && !wr[hi]) ? (hi + 3) / 4 * 4 : hi;
        for (int c = lo; c < hi; ++c) wr[c] = 1;
        return limit;
    };
    // ops executed by kernels that only know fp32 NCHW pin their tensors to it
    auto pin_fp32 = [&](const BlobOp &op) {
        for (uint32_t j = 0; j < op.n_src; ++j) cand[op.src[j].tensor] = 0;
        cand[op.dst] = 0;
    };

    steps.clear();
    steps.reserve(2 * p->net.ops.size());   // at most two steps per op: no reallocation while a Step & is held
    auto push = [&](StepKind kind, size_t i) -> Step & {
        Step &st = steps.emplace_back();
        memset(&st, 0, sizeof(st));
        st.kind = kind; st.op = (int)i;
        const BlobOp &o = p->net.ops[i];
        const Dims out = o.kind == OP_HEAD ? d[o.src[0].tensor] : d[o.dst];
        if (tags) snprintf(st.tag, sizeof(st.tag), "%02zu %s %u->%u %dx%d", i, p->net.tensors[o.dst].name, o.cin, o.cout, out.h, out.w);
        return st;
    };
    // a step of op i running convolution ci over the ranges ko
    auto conv_step = [&](size_t i, size_t ci, const KOrder &ko, const Dims &in, const Dims &out) -> Step & {
        Step &st = push(S_CONV, i);
        const BlobOp &o = p->net.ops[ci];
        ConvArgs &a = st.u.c;
        st.ci = (int)ci; st.dst_t = o.dst;
        set_sources(a, ko, tref);
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
    };
    // its kernels (conv_select.cpp: decide_conv) and what it can read / write as S4
    auto choose = [&](Step &st, int need) {
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
    };
    // pf_set_option("fuse_upsample", 0/1); at B=4: transUp.3 + conv1x1_up.3 144 us fused vs 233 us as two passes
    const bool fuse_up = p->opt.fuse_upsample != 0;   // option "fuse_upsample"
    auto can_commute_upsample = [&](size_t i, const Dims &in, const Dims &out) -> bool {
        if (!fuse || !fuse_up || i + 1 >= p->net.ops.size()) return false;
        const BlobOp &o = p->net.ops[i], &n = p->net.ops[i + 1];
        return n.kind == OP_CONV && n.k == 1 && n.stride == 1 && n.n_src == 2 && n.src[0].tensor == o.dst &&
               n.src[0].choff == 0 && n.src[0].ch == p->net.tensors[o.dst].channels && p->readers[o.dst] == 1 &&
               (in.w & 3) == 0 && (out.w & 3) == 0 && n.cout <= p->net.tensors[o.dst].channels &&
               2 * in.h <= out.h + 1 && 2 * in.w <= out.w + 1;   // >= ~2x upsampling: the residual window of a tile stays small
    };

    // ---- 2. one walk over the ops: fusions (front, pool, commuted upsample) and each convolution's choice
    cand[input] = 0;
    for (size_t i = 0; i < p->net.ops.size(); ++i) {
        const BlobOp &o = p->net.ops[i];
        const Dims in = d[o.src[0].tensor];
        const Dims out = o.kind == OP_HEAD ? in : d[o.dst];
        if (o.kind == OP_STEM && stem) {
            StemArgs a = *stem;
            a.w = p->dev_weights + p->conv[i].raw_off; a.wdep = p->dev_weights + p->conv[i].dep_off;
            a.woh = p->conv[i].oh_off ? p->dev_weights + p->conv[i].oh_off : nullptr; a.bias = p->dev_weights + p->conv[i].bias_off;
            a.status = status_of(o.dst); a.range_slot = slot_of(i, o.dst);
            a.lut = p->dev_lut; a.dst = tptr(o.dst); a.Hout = out.h; a.Wout = out.w;
            // stem -> [3x3 s1 16 -> 24] -> [3x3 s2 24 -> <= 32] with single readers: the two convs run as conv_front.hip on the
            // packed-pair stem output; the tensor between them is never stored
            bool front = false;
            if (s4_allowed && p->opt.fuse_front && i + 2 < p->net.ops.size()) {
                const BlobOp &n1 = p->net.ops[i + 1], &n2 = p->net.ops[i + 2];
                front = n1.kind == OP_CONV && n1.k == 3 && n1.stride == 1 && n1.n_src == 1 && n1.src[0].tensor == o.dst && n1.src[0].choff == 0 &&
                        n1.src[0].ch == p->net.tensors[o.dst].channels && n1.dst_choff == 0 && n1.cout == p->net.tensors[n1.dst].channels &&
                        p->readers[o.dst] == 1 && p->readers[n1.dst] == 1 && n1.relu && p->conv[i + 1].s4_off && p->conv[i + 1].s4_rounds == 2 &&
                        n2.kind == OP_CONV && n2.k == 3 && n2.stride == 2 && n2.n_src == 1 && n2.src[0].tensor == n1.dst && n2.src[0].choff == 0 &&
                        n2.src[0].ch == n1.cout && p->conv[i + 2].front_off && (n2.dst_choff & 3) == 0 &&
                        conv_front_supports((int)o.cout, (int)n1.cout, (int)n2.cout, out.h, out.w, (int)p->net.tensors[n2.dst].channels) && stem_writes_s4(a) && !conv_forced();
            }
            if (!front) {
                if (o.cout != 16 || o.k != 3 || o.stride != 2 || o.dst_choff != 0 ||
                    p->net.tensors[o.dst].channels != 16 || (uint32_t)(a.T * (a.n_cls + 1)) != o.cin)
                    return fail(PF_EUNSUPPORTED, "fused stem expects a 3x3/s2 conv %d->16, got %u->%u k%u s%u",
                                a.T * (a.n_cls + 1), o.cin, o.cout, o.k, o.stride);
                push(S_STEM, i).u.sf.stem = a;
                pin_fp32(o);
                continue;
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
        } else if (o.kind == OP_STEM || o.kind == OP_CONV) {
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
        } else if (o.kind == OP_UPSAMPLE && can_commute_upsample(i, in, out)) {
            // TransitionUp + 1x1 conv over cat([up(x), skip])  ==  W_skip*skip + up(W_x*x)   (conv_epilogue.h)
            const BlobOp &n = p->net.ops[i + 1];
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
        } else if (o.kind == OP_HEAD) {
            pin_fp32(o);
            Step &st = push(S_HEAD, i);
            HeadArgs &a = st.u.head.h;
            a.logits = tptr(o.src[0].tensor);
            a.out_seg = out_seg; a.out_logits = out_logits; a.out_is_i64 = out_seg_is_i64;
            a.B = B; a.C = (int)o.cin; a.Hin = in.h; a.Win = in.w; a.Hout = out_h; a.Wout = out_w;
            st.u.head.orig = out_orig; st.u.head.orig_bytes = (size_t)B * a.C * in.h * in.w * sizeof(float);
        } else {   // OP_POOL, OP_UPSAMPLE
            pin_fp32(o);
            PlainArgs &x = push(o.kind == OP_POOL ? S_POOL : S_UPSAMPLE, i).u.x;
            x.src = tptr(o.src[0].tensor); x.dst = tptr(o.dst); x.planes = B * (int)o.cin;
            x.hin = in.h; x.win = in.w; x.hout = out.h; x.wout = out.w;
            x.status = status_of(o.dst); x.slot = slot_of(i, o.dst);
        }
    }

    // ---- 3. formats, a fixpoint: a launch reads S4 only if ALL the ranges it accumulates are S4; a tensor stays S4 only while
    //      all its readers do and all its writers can
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
    std::vector<uint8_t> read_s4(nT, 0);
    for (const Step &r : steps)
        if (r.kind == S_CONV)
            for (int j = r.sb; j < r.se; ++j) read_s4[r.src_t[j]] = 1;
    for (size_t t = 0; t < nT; ++t) fmt[t] = cand[t] && read_s4[t];

    // ---- 4. each convolution's kernel: S4 sources, or its fp32-source kernel where that one has a kernel for the launch, else conv_dma
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
        if ((a.Win & 3) != 0) {
            if (st.need) return fail(PF_EUNSUPPORTED, "fused conv on a width that is not a multiple of 4");
            a.wpk = p->dev_weights + cp.wpk_off; a.nchunks = cp.tiling.nchunks;
            st.kind = S_CONV_GENERIC; continue;
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
            if (o.k == 1 ? conv_split1_supported(a, ch.split_nt()) : conv_split_supported(a)) continue;
            ch = ConvChoice::dma();
        }
        if (ch.is(CONV_WAVE)) {
            use(cp.wave_off, cp.wave_chunks, wave_kc((int)o.k));
            ch = ConvChoice::wave(ch.wave_mh(), ch.wave_nt() < a.ntiles ? ch.wave_nt() : a.ntiles, ch.wave_wk());
            st.kind = S_CONV_WAVE;
            if (conv_wave_supported(a, (int)o.k, ch.wave_mh(), ch.wave_nt(), ch.wave_wk())) continue;
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
                continue;
            }
        }
        conv_dma_supported(a, (int)o.k, (int)o.stride, B, ch.dma_wm(), ch.dma_nt(), p->opt.table_batch, &wm, &nt);   // (no kernel: the launcher says so)
        ch = ConvChoice::dma(wm, nt);
    }

    // ---- 5. an odd HarDBlock layer inside its consumer (conv_pair.hip): two adjacent steps P = op i, C = op i + 1 that both read
    //      and write packed pairs become one; or (conv_s4.hip share / add) stay two launches that read their common source S once: P's
    //      launch also sums C's rows over S, C's launch runs over its other ranges and adds them
    size_t w = 0;
    for (size_t k = 0; k < steps.size(); ++k, ++w) {
        const size_t i = (size_t)steps[k].op;
        // (reading S4 implies a width % 4 == 0 and no forced kernel but conv_s4)
        const bool adjacent = k + 1 < steps.size() && steps[k].kind == S_CONV_S4 && steps[k + 1].kind == S_CONV_S4 && steps[k + 1].op == (int)i + 1 &&
                              is_conv_pair(p->net, i) && steps[k].u.c.dst_fmt && steps[k + 1].u.c.dst_fmt;
        const bool pair = p->opt.fuse_pairs && adjacent && p->conv[i + 1].pair_c_off;
        const BlobOp &o = p->net.ops[i];
        if (!pair || !pair_wanted((int)o.cin, (int)o.cout, (int)p->net.ops[i + 1].cin, (int)p->net.ops[i + 1].cout, d[o.dst].h, d[o.dst].w, Bt,
                                  p->opt.fuse_pairs)) {
            // share / add: 8 x 32 tiles without a K split for both launches, packings made at plan creation
            if (adjacent && p->opt.share_s && p->conv[i + 1].share_a_off && share_off != (size_t)-1 && steps[k].dec.s4_tile == S4_8x32 && steps[k + 1].dec.s4_tile == S4_8x32 &&
                share_wanted((int)o.cin, (int)o.cout, (int)p->net.ops[i + 1].cin, (int)p->net.ops[i + 1].cout, d[o.dst].h, d[o.dst].w, Bt, p->opt.share_s)) {
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
                set_sources(c, order_add(p->net.ops[i + 1].src, (int)p->net.ops[i + 1].n_src), tref);
                c.Cin = c.src_cstart[c.n_src];
                c.wpk = p->dev_weights + cc.share_b_off; c.nchunks = cc.share_b_rounds;
                set_s4_entries(c, 3, 0);
                c.share = sums; c.share_cout = c.Cout;
                steps[w] = sa;
                steps[++w] = sb;
                ++k;
                continue;
            }
            if (w != k) steps[w] = steps[k];
            continue;
        }
        // the consumer's S4 launch (pa.c) with its sources in the pair's K order [S, others.., P]
        const BlobOp &C = p->net.ops[i + 1];
        Step st = steps[k + 1];
        st.kind = S_PAIR; st.op = (int)i;
        if (tags)
            snprintf(st.tag, sizeof(st.tag), "%02zu+%02zu %s+%s %u->%u->%u %dx%d", i, i + 1, p->net.tensors[o.dst].name, p->net.tensors[C.dst].name, o.cin,
                     o.cout, C.cout, d[o.dst].h, d[o.dst].w);
        PairArgs &pa = st.u.pair;
        ConvArgs &a = pa.c;
        const int n = (int)C.n_src;
        set_sources(a, order_pair(C.src, n), tref);
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
        steps[w] = st;
        ++k;
    }
    steps.resize(w);

    // ---- 6. the folds of conv_s4.hip, one form after the other: a 3x3 conv L and the 1x1 conv R that reads its slice last (is_conv_fold) as
    //      ONE launch.  Two adjacent plain conv_s4 steps - not part of a pair or a share / add step, whose kinds differ -, L on
    //      <2, 32, 8, 1> or, the wide forms, <3, 32, 8, 1> into packed pairs; R's step goes away.  (up: R's step is the low-resolution half of
    //      the commuted upsample + 1x1 conv, made under the upsample's op; the other half stays as it is)
    auto fold = [&](FoldForm form) {
        const FoldDesc &f = kFolds[form];
        const int mode = p->opt.*f.option;
        for (size_t k = 0; mode && p->fold[form].dev && k + 1 < steps.size(); ++k) {
            Step &sl = steps[k];
            const Step &sr = steps[k + 1];
            const size_t i = (size_t)sl.op;
            if (sl.kind != S_CONV_S4 || sr.kind != S_CONV_S4 || sl.ci != (int)i || sr.op != (int)i + 1 || sr.ci != (int)(i + f.r_at())) continue;
            if (!p->conv[i].fold_off[form] || !is_conv_fold(p->net, i, form)) continue;
            const BlobOp &L = p->net.ops[i], &R = p->net.ops[i + f.r_at()];
            ConvArgs &a = sl.u.c;
            const ConvArgs &r = sr.u.c;
            const S4Shape &sh = sl.dec.s4;
            if (sh.NT != f.l_tiles || sh.TW != 32 || sh.TH != 8 || sh.KS != 1 || !a.dst_fmt || r.res || a.Hout != r.Hout || a.Wout != r.Wout) continue;
            // tail: R without fused stages into fp32, nothing of it range-checked.  down: R with its pool fused and nothing else, into
            // packed pairs or fp32.  lo: the first range of R alone, without bias or ReLU, into fp32
            if (f.up ? (!r.no_bias || r.relu || r.src_begin != 0 || r.src_end != 1 || r.dst_fmt || r.status || r.pool)
                     : r.no_bias || (form == FOLD_TAIL ? (r.dst_fmt || r.status || r.pool) : (!r.pool || !r.relu)))
                continue;
            if (!f.wanted((int)L.cin, (int)L.cout, (int)R.cout, a.Hout, a.Wout, Bt, mode)) continue;
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
            steps.erase(steps.begin() + (long)k + 1);
        }
    };
    for (int form = 0; form < kFoldForms; ++form) fold((FoldForm)form);
    return PF_OK;
}

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
