// bg training step, host only: the net as a training plan holds it (op table, parameter layout), who writes a tensor's gradient
// first, and where everything of a step lives in the workspace.
//
// Parameters live in ONE flat fp32 arena `theta` (the Python side maps the reference's state_dict keys onto it), gradients in an
// arena of the same layout - so the data-parallel exchange is a single all-reduce of ~16.5 MB over RCCL between
// pf_train_forward_backward and pf_sgd_step (the reference wraps the model in DDP, train.py:96-103).
//
// theta layout: for every conv op of the table, in table order:  W[cout][cin][k][k],  then
//     with BatchNorm:  gamma[cout], beta[cout], running_mean[cout], running_var[cout]      (ConvLayer, hardnet.py:16-25)
//     without       :  bias[cout]                                                          (finalConv, hardnet.py:325-327)
#include "train_plan.h"

namespace pf {

int train_net_init(const void *blob, size_t bytes, int in_ch, int n_cls, TrainNet &n) {
    if (int rc = parse_net_table(blob, bytes, in_ch, n_cls, n.net)) return rc;
    const size_t n_ops = n.net.ops.size();
    n.w_off.assign(n_ops, 0);
    n.aux_off.assign(n_ops, 0);
    n.bn.assign(n_ops, 0);
    size_t cur = 0;
    for (size_t i = 0; i < n_ops; ++i) {
        const BlobOp &o = n.net.ops[i];
        if (!is_conv(o.kind)) continue;
        uint32_t cin = 0;
        for (uint32_t j = 0; j < o.n_src; ++j) cin += o.src[j].ch;
        if (cin != o.cin || !((o.k == 3 && (o.stride == 1 || o.stride == 2)) || (o.k == 1 && o.stride == 1)))
            return fail(PF_EUNSUPPORTED, "op %zu: training supports 3x3 (stride 1/2) and 1x1 convs", i);
        // packing.py writes pad[0] = 1 + has_bn; blobs without the field: ConvLayer (conv + BN + ReLU) <=> relu flag
        n.bn[i] = o.pad[0] ? (int)o.pad[0] - 1 : (int)(o.relu != 0);
        n.w_off[i] = cur;
        cur += (size_t)o.cout * o.cin * o.k * o.k;
        n.aux_off[i] = cur;
        cur += (size_t)o.cout * (n.bn[i] ? 4 : 1);
    }
    n.n_params = cur;
    n.fwd_s4 = g_opt_train_s4;
    n.side = g_opt_train_side != 0;
    return PF_OK;
}

GradFirst grad_first_writers(const TrainNet &n, const std::vector<Dims> &d) {
    const NetTable &net = n.net;
    GradFirst g;
    g.store.assign(net.ops.size(), std::array<uint8_t, kConvMaxSrc>{});
    const uint32_t input = net.ops[0].src[0].tensor;
    std::vector<std::vector<uint8_t>> touched(net.tensors.size());
    for (size_t t = 0; t < net.tensors.size(); ++t) touched[t].assign(net.tensors[t].channels, 0);
    auto clear_fresh = [&](uint32_t t, uint32_t c0, uint32_t nc) {       // the runs of channels in [c0, c0 + nc) nobody has written yet
        for (uint32_t c = c0; c < c0 + nc;) {
            if (touched[t][c]) { ++c; continue; }
            uint32_t e = c;
            while (e < c0 + nc && !touched[t][e]) ++e;
            g.clear.push_back({(int)t, (int)c, (int)(e - c)});
            c = e;
        }
    };
    for (size_t ii = net.ops.size(); ii-- > 0;) {
        const BlobOp &o = net.ops[ii];
        const bool whole = !is_conv(o.kind);      // pool / upsample / head write the whole tensor
        const uint32_t nj = whole ? 1 : o.n_src;
        for (uint32_t j = 0; j < nj; ++j) {
            const uint32_t t = o.src[j].tensor;
            if (t == input) continue;
            const uint32_t c0 = whole ? 0 : o.src[j].choff, nc = whole ? net.tensors[t].channels : o.src[j].ch;
            uint32_t fresh = 0;
            for (uint32_t c = c0; c < c0 + nc; ++c) fresh += !touched[t][c];
            if (fresh == nc) g.store[ii][j] = 1;
            else if (fresh) clear_fresh(t, c0, nc);
            for (uint32_t c = c0; c < c0 + nc; ++c) touched[t][c] = 1;
        }
    }
    for (size_t t = 0; t < net.tensors.size(); ++t)
        if (t != input && d[t].h) clear_fresh((uint32_t)t, 0, net.tensors[t].channels);
    return g;
}

// may op i's forward convolution run on conv_s4?  conv + BatchNorm, 3x3 / 1x1, stride 1, every input range at an even channel of a
// tensor some op produced (the network input stays dense fp32: the stem reads it)
static bool s4_fwd_ok(const TrainNet &n, size_t i) {
    const BlobOp &o = n.net.ops[i];
    if (!n.fwd_s4 || o.kind != OP_CONV || !n.bn[i] || o.stride != 1 || (o.k != 1 && o.k != 3) || o.n_src > (uint32_t)kConvMaxSrc) return false;
    const uint32_t input = n.net.ops[0].src[0].tensor;
    for (uint32_t j = 0; j < o.n_src; ++j)
        if ((o.src[j].choff & 1) || o.src[j].tensor == input) return false;
    return true;
}

TLayout t_layout(const TrainNet &n, bool autotune, int B, const std::vector<Dims> &d, int out_h, int out_w, std::vector<TRegion> *regions) {
    const NetTable &net = n.net;
    TLayout L;
    const size_t nt = net.tensors.size(), n_ops = net.ops.size();
    L.act.assign(nt, (size_t)-1);
    L.grad.assign(nt, (size_t)-1);
    L.ypre.assign(n_ops, (size_t)-1);
    L.stat.assign(n_ops, (size_t)-1);
    L.xpad.assign(n_ops, (size_t)-1);
    size_t cur = 0;
    auto take = [&](size_t bytes, TRegionKind kind, size_t index = 0) {
        const size_t o = cur;
        cur += align_up(bytes, 256);
        if (regions) regions->push_back({kind, (int)index, o, bytes});
        return o;
    };
    auto tbytes = [&](size_t t) { return (size_t)B * net.tensors[t].channels * d[t].h * d[t].w * sizeof(float); };
    for (size_t t = 0; t < nt; ++t)
        if (d[t].h) L.act[t] = take(tbytes(t), R_ACT, t);
    const uint32_t input = net.ops[0].src[0].tensor;
    for (size_t t = 0; t < nt; ++t)
        if (d[t].h && t != input) L.grad[t] = take(tbytes(t), R_GRAD, t);
    L.odd.assign(n_ops, 0);
    size_t max_dy = 0, max_wpart = 0, max_c = 16, max_pad = 256;
    for (size_t i = 0; i < n_ops; ++i) {
        const BlobOp &o = net.ops[i];
        if (!is_conv(o.kind)) continue;
        const Dims in = d[o.src[0].tensor], out = d[o.dst];
        L.odd[i] = (in.w & 3) && o.stride == 1;
        // the conv output (y, dy) in padded rows on an odd level
        const size_t ybytes = (size_t)B * o.cout * out.h * (L.odd[i] ? round_up4(out.w) : out.w) * sizeof(float);
        if (n.bn[i]) {
            L.ypre[i] = take(ybytes, R_YPRE, i);
            L.stat[i] = take(2 * (size_t)o.cout * sizeof(float), R_STAT, i);
        }
        // dy scratch: the conv-output gradient, and (stride 2) its zero-stuffed copy at the input resolution
        size_t need = ybytes;
        if (o.stride == 2) need += align_up((size_t)B * o.cout * in.h * in.w * sizeof(float), 256);
        max_dy = need > max_dy ? need : max_dy;
        if (L.odd[i]) L.xpad[i] = take((size_t)B * o.cin * in.h * round_up4(in.w) * sizeof(float), R_XPAD, i);
        if (in.w & 3) {     // padded copies (forward: cin -> cout at the output size; backward-data: cout -> cin at the input size)
            const size_t cmax = o.cin > o.cout ? o.cin : o.cout;
            const size_t bytes = (size_t)B * cmax * in.h * round_up4(in.w) * sizeof(float);
            max_pad = bytes > max_pad ? bytes : max_pad;
        }
        const int wpi = o.stride == 1 ? round_up4(in.w) : in.w, wpo = o.stride == 1 ? round_up4(out.w) : out.w;   // (padded copies for odd widths)
        const size_t wp = wgrad_partial_floats((int)o.cout, (int)o.cin, (int)o.k, B, out.h, wpi, wpo);
        max_wpart = wp > max_wpart ? wp : max_wpart;
        max_c = o.cout > max_c ? o.cout : max_c;
    }
    // the step's packing jobs (the padded copies of odd-width levels read ONE gathered range)
    {
        L.fwd_job.assign(n_ops, -1);
        L.bwd_job.assign(n_ops, std::vector<int>());
        L.bwd_all_job.assign(n_ops, -1);
        size_t arena = 0;
        auto add = [&](size_t i, int stride, const int *chs, int ns, int tflip, int c0, int ch) {
            const BlobOp &o = net.ops[i];
            PackJob q;
            pack_job_fill(q, n.w_off[i], (int)o.cin, (int)o.cout, (int)o.k, stride, chs, ns, tflip, c0, ch, arena);
            arena += align_up((size_t)q.total, 64);
            L.jobs.push_back(q);
            return (int)L.jobs.size() - 1;
        };
        for (size_t i = 0; i < n_ops; ++i) {
            const BlobOp &o = net.ops[i];
            if (!is_conv(o.kind)) continue;
            int src_ch[kConvMaxSrc];
            for (uint32_t j = 0; j < o.n_src; ++j) src_ch[j] = (int)o.src[j].ch;
            const int one = (int)o.cin;
            const bool aligned = (d[o.src[0].tensor].w & 3) == 0;
            L.fwd_job[i] = add(i, (int)o.stride, aligned ? src_ch : &one, aligned ? (int)o.n_src : 1, 0, 0, 0);
        }
        for (size_t i = 0; i < n_ops; ++i) {
            const BlobOp &o = net.ops[i];
            if (!is_conv(o.kind)) continue;
            L.bwd_job[i].assign(o.n_src, -1);
            const int dy_ch = (int)o.cout;
            if (L.odd[i]) {
                L.bwd_all_job[i] = add(i, 1, &dy_ch, 1, 1, 0, (int)o.cin);
                continue;
            }
            const KOrder ko = order_plain(o.src, (int)o.n_src);
            for (int j = 0; j < ko.n; ++j)
                if (ko.r[j].tensor != input) L.bwd_job[i][j] = add(i, 1, &dy_ch, 1, 1, ko.r[j].cstart, ko.r[j].ch);
        }
        L.wpk_arena = take(arena * sizeof(float) + 256, R_WPK);
    }
    // the forward convolutions that run on the packed-pair kernels: their device-side weight packings, and the shadows of the tensors they read
    {
        L.s4act.assign(nt, (size_t)-1);
        L.s4_job.assign(n_ops, -1);
        std::vector<char> need(nt, 0);
        size_t arena = 0;
        for (size_t i = 0; i < n_ops; ++i) {
            if (!s4_fwd_ok(n, i)) continue;
            const BlobOp &o = net.ops[i];
            for (uint32_t j = 0; j < o.n_src; ++j) need[o.src[j].tensor] = 1;
            S4WJob jb;
            const size_t fl = s4_wjob_init(jb, n.w_off[i], (int)o.cin, (int)o.cout, (int)o.k, order_plain(o.src, (int)o.n_src), o.k == 1 && o.n_src == 2);
            jb.out_off = (unsigned)arena;
            arena += align_up(fl, 64);
            L.s4_job[i] = (int)L.s4jobs.size();
            L.s4jobs.push_back(jb);
        }
        for (size_t t = 0; t < nt; ++t)
            if (need[t] && d[t].h) L.s4act[t] = take((size_t)B * 2 * ((net.tensors[t].channels + 3) / 4) * d[t].h * round_up4(d[t].w) * 8, R_S4ACT, t);
        L.s4w_arena = take(arena * sizeof(float) + 256, R_S4W);
    }
    if (autotune) L.tune_grad = take(n.n_params * sizeof(float), R_TUNE_GRAD);
    L.dy = take(max_dy + 256, R_DY);
    if (n.side)
        for (int k = 1; k < kDySlots; ++k) L.dy_more[k] = take(max_dy + 256, R_DY, k);
    L.wpart = take(max_wpart * sizeof(float), R_WPART);
    if (n.side)
        for (int k = 1; k < kSideStreams; ++k) L.wpart_more[k] = take(max_wpart * sizeof(float), R_WPART, k);
    L.pad_in = take(max_pad, R_PAD_IN);
    L.pad_out = take(max_pad, R_PAD_OUT);
    L.dfull = take((size_t)B * net.hdr.n_cls * out_h * out_w * sizeof(float), R_DFULL);
    {
        size_t mx = 0;
        for (const BlobOp &o : net.ops) {
            const Dims in = d[o.src[0].tensor];
            size_t fl = 0;
            if (o.kind == OP_HEAD) fl = upsample_bwd_tmp_floats(B * (int)o.cin, in.h, in.w, out_h, out_w);
            else if (o.kind == OP_UPSAMPLE) fl = upsample_bwd_tmp_floats(B * (int)o.cin, in.h, in.w, d[o.dst].h, d[o.dst].w);
            mx = fl > mx ? fl : mx;
        }
        L.up_tmp = take(mx * sizeof(float) + 256, R_UP_TMP);
    }
    L.cepart = take(ce_partial_doubles(B, out_h, out_w) * sizeof(double), R_CEPART);
    L.bnpart = take(bn_partial_doubles((int)max_c) * sizeof(double), R_BNPART);
    L.out3 = take(4 * sizeof(double), R_OUT3);
    L.total = cur;
    if (regions) regions->push_back({R_TOTAL, 0, 0, cur});
    return L;
}

}  // namespace pf
