// bg training step, host only: build_train_schedule - the whole step as a flat list of TSteps, each naming exactly one kernel or
// stream operation with all of its arguments; every kernel and shape is chosen here through predicates, so a geometry without a
// kernel fails before anything is enqueued.  And pf_debug_train_plan, which hands layout and schedule to tests without a device.
//
// Convolutions run on the fp32 matrix cores: forward and backward-data through the LDS-DMA kernels of the inference path
// (conv_dma.hip; widths that are not a multiple of 4 on copies with padded rows) with the weights re-packed on the device
// every step (forward order, or transposed + flipped per input range; stride-2 backward-data = stride-1 conv over the
// zero-stuffed gradient; a tensor's gradient accumulates over its consumers in the store), backward-weight through the
// LDS-tiled wgrad kernels of train_wgrad.hip.
#include <algorithm>
#include <cstring>

#include "pf_prof.h"
#include "train_plan.h"

namespace pf {

// measured shapes of the training step's convolutions for the configurations tools/tune_train.py was run on (the reference's
// configs/bg/bg_train.yaml: batch 8 of 800x800 crops): {ks, stride, Cin, Cout, Hin, Win, B, accum, wm, nt}.  Consulted when option
// "use_tuned_table" is on (default) and the plan does not measure for itself; other geometries take the cost model's shape
struct TrainTuned { int key[8], wm, nt; };
static const TrainTuned kTrainTuned[] = {
#include "train_tuned.inc"
    {{0, 0, 0, 0, 0, 0, 0, 0}, 0, 0}};

// conv `c` reading ONE source instead of its ranges: all `cin` channels of buffer x, rows of `win` pixels (the gathered copy of an
// odd-width conv, the backward-data convs over dy)
static ConvArgs over_buffer(ConvArgs c, const float *x, int cin, int win, int wout) {
    const BlobSrc all{0, 0, (uint32_t)cin};
    set_sources(c, order_plain(&all, 1), [&](uint32_t) { return TensorRef{x, cin}; });
    c.Cin = cin; c.Win = win; c.Wout = wout;
    return c;
}

int build_train_schedule(const TrainNet &n, const TCall &k, const std::vector<Dims> &d, const TLayout &L, const GradFirst &gfirst,
                         const float *zero_page, const TunedMap *tuned, bool measuring, std::vector<TStep> &steps) {
    const NetTable &net = n.net;
    // the options read per call
    const int kacc = g_opt_train_kacc, use_tuned = g_plan_opt.use_tuned_table, table_batch = g_opt_train_table_batch;
    const bool tagged = prof_enabled();
    const int B = k.B;
    char *wsb = (char *)k.ws;
    auto buf = [&](size_t off) { return reinterpret_cast<float *>(wsb + off); };
    auto act = [&](uint32_t t) { return buf(L.act[t]); };
    auto channels = [&](uint32_t t) { return (int)net.tensors[t].channels; };
    auto act_ref = [&](uint32_t t) { return TensorRef{act(t), channels(t)}; };
    auto gradt = [&](uint32_t t) { return buf(L.grad[t]); };
    const uint32_t input = net.ops[0].src[0].tensor;
    const int in_ch = channels(input), n_cls = (int)net.hdr.n_cls;
    float *dy_slot[kDySlots];
    for (int j = 0; j < kDySlots; ++j) dy_slot[j] = buf(n.side && j ? L.dy_more[j] : L.dy);
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
        a.bias = a.zero_page = zero_page;
        a.Cin = (int)o.cin; a.Cout = (int)o.cout; a.ntiles = ((int)o.cout + 15) / 16;
        a.Hin = in.h; a.Win = in.w; a.Hout = out.h; a.Wout = out.w;
        return a;
    };
    // backward-data conv: `ch` gradient channels into dst from the cout_f channels of dy ([B][cout_f][h][w])
    auto bwd_data_args = [&](const float *dy, int cout_f, int ch, int h, int w, float *dst, int dst_ctotal, int dst_choff, int accum) {
        ConvArgs b;
        memset(&b, 0, sizeof(b));
        b.bias = b.zero_page = zero_page;
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
        const std::pair<int, int> *measured = tuned && tuned->count(key) ? &tuned->at(key) : nullptr;
        if (forced_dma_shape(&wm, &nt)) {
            // pf_debug_force_conv(1, wm, nt, 0): every conv_dma step of the schedule with that shape (conv_dma_supported clamps nt to
            // the layer's cout tiles); counted in none of the path statistics' table / cost-model / measured slots
            src = 3;
        } else if (measured) {
            wm = measured->first, nt = measured->second, src = 2;
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
        TStep &st = add(src == 2 && !measured ? T_CONV_DMA_MEASURE : T_CONV_DMA, stats | (uint8_t)(src < 3 ? 1u << src : 0u));
        TConvArgs &x = st.u.conv;
        x.a = c; x.ks = ks; x.stride = stride;
        if (st.kind == T_CONV_DMA && !conv_dma_supported(c, ks, stride, B, wm, nt, 0, &x.wm, &x.nt))
            return fail(PF_EUNSUPPORTED, "training: conv_dma has no kernel for ks=%d stride=%d wm=%d nt=%d", ks, stride, x.wm, x.nt);
        return PF_OK;
    };
    // the gathered, row-padded copy of the input ranges of `a` (path stats 3; 4: the conv keeps its output in padded rows)
    auto pad_gather = [&](const ConvArgs &a, int Wp, float *to, bool keep_padded) { add(T_PAD_GATHER, keep_padded ? 0x18 : 0x08).u.gather = {a, Wp, to}; };
    // one convolution on conv_dma.  Odd width: the same kernel on the input ranges gathered into `gather` with rows padded to a
    // multiple of 4; the output left in padded rows at a.dst (keep_padded: the BatchNorm kernels read that pitch) or scattered
    // back from pad_out
    auto conv = [&](const ConvArgs &a, int ks, int stride, int job, float *gather, bool keep_padded) -> int {
        if ((a.Win & 3) == 0) return dma(a, ks, stride, job, 0);
        const int Wp = round_up4(a.Win), Wop = (Wp + 2 * (ks / 2) - ks) / stride + 1;
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
    std::vector<std::vector<char>> s4_written(net.tensors.size());
    auto shadow = [&](uint32_t t, int c0, int c1) {
        if (L.s4act[t] == (size_t)-1) return;
        const int ct = channels(t);
        std::vector<char> &wr = s4_written[t];
        if (wr.empty()) wr.assign((size_t)ct + 4, 0);
        const int fill_lo = (c0 & 2) && !wr[c0 - 2], fill_up = (c1 & 3) == 2 && c1 < ct && !wr[c1];
        for (int c = c0; c < c1; ++c) wr[c] = 1;
        add(T_S4_ACT).u.s4act = {act(t), ct, c0, c1, fill_lo, fill_up, d[t].h, d[t].w, round_up4(d[t].w), wsb + L.s4act[t]};
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
        add(T_ZERO_CHANNELS).u.zch = {gradt((uint32_t)c[0]), channels((uint32_t)c[0]), c[1], c[2], (long long)d[c[0]].h * d[c[0]].w};
    if (!k.accumulate_grads) add(T_ZERO_FILL).u.copy = {k.grad, nullptr, n.n_params * sizeof(float)};

    // ================================================================ forward (training mode)
    for (size_t i = 0; i < net.ops.size(); ++i) {
        const BlobOp &o = net.ops[i];
        const Dims in = d[o.src[0].tensor];
        const Dims out = o.kind == OP_HEAD ? in : d[o.dst];
        if (is_conv(o.kind)) {
            ConvArgs a = conv_args(o, in, out);
            float *gather = L.odd[i] ? buf(L.xpad[i]) : pad_in;     // (an odd op keeps its copy for the weight gradient)
            const int Wp = round_up4(in.w);
            if (!n.bn[i]) {
                a.bias = k.theta + n.aux_off[i];
                a.dst = act(o.dst); a.dst_ctotal = channels(o.dst); a.dst_choff = (int)o.dst_choff; a.relu = (int)o.relu;
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
                TConvArgs &x = add(T_CONV_S4, 0x80).u.conv;
                ConvArgs &c = x.a = a;
                set_sources(c, order_plain(o.src, (int)o.n_src), [&](uint32_t t) { return TensorRef{buf(L.s4act[t]), channels(t)}; });
                c.src_fmt = 1; c.dst_fmt = 0;
                c.Win = Wp; c.Wout = Wp;
                c.acc_scale = 1.0f / (kS4TrainWeightScale * kS4TrainActScale);
                c.wpk = buf(L.s4w_arena) + jb.out_off;
                c.nchunks = jb.rounds;
                set_s4_entries(c, (int)o.k, jb.pad);
                c.kacc = (kacc && o.k == 3) ? 1 : 0;      // blocked summation, as in the fp32 step (conv_s4_kernel.inc: KACC)
                x.ks = (int)o.k;
                int nt = c.ntiles == 3 ? 3 : (c.ntiles < 2 ? 1 : 2), tile = S4_8x32;   // unless the layer's measured row names a shape
                ConvChoice row;
                if (use_tuned && choose_s4((int)o.k, c.Cin, c.Cout, c.Hout, c.Wout, B, &row) && row.is(CONV_S4)) { nt = row.s4_nt(); tile = row.s4_tile(); }
                x.s4 = s4_resolve(x.ks, nt, tile, c.ntiles, c.nchunks, c.kacc != 0);
            }
            float *aux = k.theta + n.aux_off[i], *stat = buf(L.stat[i]);
            add(T_BN_FWD).u.bnf = {y, (int)o.cout, out.h, out.w, k.bn_eps, k.bn_momentum, aux, aux + o.cout,
                                   k.update_running_stats ? aux + 2 * o.cout : nullptr, k.update_running_stats ? aux + 3 * o.cout : nullptr,
                                   stat, stat + o.cout, bnpart, act(o.dst), channels(o.dst), (int)o.dst_choff, (int)o.relu,
                                   L.odd[i] ? round_up4(out.w) : 0};
            shadow(o.dst, (int)o.dst_choff, (int)o.dst_choff + (int)o.cout);
        } else if (o.kind == OP_POOL) {
            add(T_POOL).u.plain = {act(o.src[0].tensor), act(o.dst), B * (int)o.cin, in.h, in.w, 0, 0, 0};
            shadow(o.dst, 0, channels(o.dst));
        } else if (o.kind == OP_UPSAMPLE) {
            add(T_UPSAMPLE).u.plain = {act(o.src[0].tensor), act(o.dst), B * (int)o.cin, in.h, in.w, out.h, out.w, 0};
            shadow(o.dst, 0, channels(o.dst));
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
    for (size_t ii = net.ops.size(); ii-- > 0;) {
        const BlobOp &o = net.ops[ii];
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
        } else if (is_conv(o.kind)) {
            if (!n.bn[ii] && o.relu) return fail(PF_EUNSUPPORTED, "training: ReLU without BatchNorm (op %zu)", ii);
            float *aux = k.theta + n.aux_off[ii], *gaux = k.grad + n.aux_off[ii];
            const int slot = n_conv % kDySlots, sidx = n_conv % kSideStreams;
            float *dy = dy_slot[slot];
            // odd-width levels: dy goes out with its rows padded to a multiple of 4 floats and zero pad columns - the form the
            // tiled weight-gradient and backward-data kernels read - and ONE backward-data conv covers all input ranges
            const bool odd = L.odd[ii];
            const int Wp = round_up4(in.w), pitch = odd ? Wp : 0;
            if (n.side && n_conv >= kDySlots) add(T_WAIT_WG, 0, -1, slot);
            ++n_conv;
            if (n.bn[ii]) {
                const float *stat = buf(L.stat[ii]);
                add(T_BN_BWD).u.bnb = {gradt(o.dst), channels(o.dst), (int)o.dst_choff, buf(L.ypre[ii]), stat, stat + o.cout, aux, aux + o.cout,
                                       (int)o.cout, out.h, out.w, (int)o.relu, gaux, gaux + o.cout, bnpart, dy, pitch, pitch};
            } else {
                add(T_BIAS_BWD).u.bnb = {gradt(o.dst), channels(o.dst), (int)o.dst_choff, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         (int)o.cout, out.h, out.w, 0, gaux, nullptr, bnpart, dy, pitch, 0};
            }
            // dW (odd width: the tiled kernel on the padded copy of x the forward pass gathered and the padded dy; zero pad
            // columns add nothing)
            if (n.side) add(T_FORK, 0, sidx, slot);
            {
                TWgradArgs &x = add(T_WGRAD, 0, n.side ? sidx : -1).u.wg;
                const ConvArgs a = conv_args(o, in, out);
                x.a = odd ? over_buffer(a, buf(L.xpad[ii]), (int)o.cin, Wp, Wp) : a;
                x.ks = (int)o.k; x.stride = odd ? 1 : (int)o.stride;
                x.dy = dy; x.partial = buf(n.side && sidx ? L.wpart_more[sidx] : L.wpart); x.dw = k.grad + n.w_off[ii];
                if (tagged)      // per-layer rows of tools/bench_train.py --layers
                    snprintf(x.tag, sizeof(x.tag), "%02d %u->%u k%u s%u %dx%d", (int)ii, o.cin, o.cout, o.k, o.stride, out.h, out.w);
            }
            if (n.side) add(T_WG_DONE, 0, sidx, slot);
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
                        m.ctotal[j] = channels(o.src[j].tensor);
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
                const ConvArgs b = bwd_data_args(dsrc, (int)o.cout, (int)o.src[j].ch, in.h, in.w, gradt(t), channels(t),
                                                 (int)o.src[j].choff, gfirst.store[ii][j] ? 0 : 1);
                if ((rc = conv(b, (int)o.k, 1, L.bwd_job[ii][j], pad_in, false))) return rc;
            }
        }
    }
    return PF_OK;
}

}  // namespace pf

using namespace pf;

extern "C" int pf_debug_train_plan(const void *blob, size_t bytes, int in_ch, int n_cls, int B, int H, int W, int out_h, int out_w,
                                   long long *regions, int cap_regions, int *n_regions, int *steps, int cap_steps, int *n_steps,
                                   int *slots_streams) {
    if (!blob || !n_regions || !n_steps || (cap_regions > 0 && !regions) || (cap_steps > 0 && !steps) || B <= 0 || H <= 0 || W <= 0 ||
        out_h <= 0 || out_w <= 0)
        return fail(PF_EINVAL, "pf_debug_train_plan: bad argument");
    TrainNet net;
    std::vector<Dims> d;
    int rc = train_net_init(blob, bytes, in_ch, n_cls, net);
    if (!rc) rc = propagate_dims(net.net, H, W, d);
    if (rc) return rc;
    std::vector<TRegion> reg;
    const TLayout L = t_layout(net, false, B, d, out_h, out_w, &reg);
    // made-up addresses, far apart: the schedule computes with them and reads nothing through them
    char *const ws = (char *)(1ull << 44);
    float *const fake = (float *)(1ull << 40);
    TCall k{};
    k.theta = fake + (1ull << 36); k.grad = fake + (2ull << 36);
    k.x_dense = fake + (3ull << 36); k.labels = fake + (4ull << 36); k.out3 = (double *)(fake + (5ull << 36));
    k.B = B; k.H = H; k.W = W; k.out_h = out_h; k.out_w = out_w;
    k.loss_scale = 1.f; k.bn_momentum = 0.1f; k.bn_eps = 1e-5f; k.update_running_stats = 1;
    k.ws = ws; k.ws_bytes = L.total;
    std::vector<TStep> sched;
    if ((rc = build_train_schedule(net, k, d, L, grad_first_writers(net, d), fake, nullptr, false, sched))) return rc;
    *n_regions = (int)reg.size();
    for (size_t i = 0; i < reg.size() && (int)i < cap_regions; ++i) {
        const long long row[4] = {reg[i].kind, reg[i].index, (long long)reg[i].off, (long long)reg[i].bytes};
        std::copy(row, row + 4, regions + 4 * i);
    }
    // what a step does to tensors' gradients, read back from its pointers: the tensor whose gradient region starts at p, or -1
    std::vector<std::array<int, 5>> rows;
    auto touch = [&](const void *p, int c0, int nc, int access) {
        for (size_t t = 0; p && t < L.grad.size(); ++t)
            if (L.grad[t] != (size_t)-1 && (const char *)p == ws + L.grad[t])
                rows.push_back({1, (int)t, c0, nc < 0 ? (int)net.net.tensors[t].channels : nc, access});
    };
    enum { STORE, ADD, CLEAR, READ };
    for (const TStep &st : sched) {
        rows.push_back({0, st.kind, st.side, st.slot, st.stats});
        const auto &u = st.u;
        switch (st.kind) {
            case T_CONV_DMA: case T_CONV_DMA_MEASURE: case T_CONV_S4:
                touch(u.conv.a.dst, u.conv.a.dst_choff, u.conv.a.Cout, u.conv.a.accum ? ADD : STORE); break;
            case T_UNPAD: touch(u.unpad.dst, u.unpad.choff, u.unpad.C, u.unpad.accum ? ADD : STORE); break;
            case T_UNPAD_MULTI:
                for (int j = 0; j < u.unpadm.n; ++j) touch(u.unpadm.dst[j], u.unpadm.choff[j], u.unpadm.ch[j], u.unpadm.overwrite[j] ? STORE : ADD);
                break;
            case T_POOL_BWD: touch(u.plain.src, 0, -1, READ); touch(u.plain.dst, 0, -1, u.plain.overwrite ? STORE : ADD); break;
            case T_UPSAMPLE_BWD: touch(u.upb.gout, 0, -1, READ); touch(u.upb.gin, 0, -1, u.upb.accumulate ? ADD : STORE); break;
            case T_ZERO_CHANNELS: touch(u.zch.t, u.zch.c0, u.zch.n, CLEAR); break;
            case T_BN_BWD: case T_BIAS_BWD: touch(u.bnb.g, u.bnb.choff, u.bnb.C, READ); break;
            default: break;
        }
    }
    *n_steps = (int)rows.size();
    for (size_t i = 0; i < rows.size() && (int)i < cap_steps; ++i) std::copy(rows[i].begin(), rows[i].end(), steps + 5 * i);
    if (slots_streams) slots_streams[0] = kDySlots, slots_streams[1] = kSideStreams;
    return PF_OK;
}
