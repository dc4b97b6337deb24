// Plan creation: the blob's op table (pf_net.h) -> normalize_ranges over the folded weights -> build_plan_weights (every packing of
// every convolution in one host arena; no device involved) -> upload.  And the option table behind pf_set_option /
// pf_hardnet_plan_set_option.  Nothing about FC-HarDNet-70 is hard-coded here, so single-op test networks use the same code.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "hardnet_plan.h"

using namespace pf;

namespace pf {
PlanOptions g_plan_opt;
// process-wide only: plain globals where their readers live (train_plan.hip, train_wgrad.hip)
extern int g_opt_train_side, g_opt_wgrad_taps, g_opt_train_s4, g_opt_train_kacc, g_opt_train_table_batch, g_opt_up_two_pass;
}

namespace {

// Every option: its name (and the name round 1 gave it), where the value lives - a member of PlanOptions (of g_plan_opt, or of a
// plan's copy) or a process-wide global -, which of the two entry points accepts it, and whether negative values clamp to 0
struct Option {
    const char *name, *alias;
    int PlanOptions::*member;
    int *global;
    bool process, per_plan, clamp0;
};
const Option kOptions[] = {
    {"fuse_pool", nullptr, &PlanOptions::fuse_pool, nullptr, true, true, false},
    {"fuse_upsample", nullptr, &PlanOptions::fuse_upsample, nullptr, true, true, false},
    {"use_tuned_table", nullptr, &PlanOptions::use_tuned_table, nullptr, true, true, false},   // (its process value: also the training step)
    {"valu_remainder", nullptr, &PlanOptions::valu_remainder, nullptr, true, true, false},
    {"split_f16", "split_bf16", &PlanOptions::split_f16, nullptr, true, true, false},
    {"packed_acts", nullptr, &PlanOptions::packed_acts, nullptr, true, true, false},
    {"range_guard", nullptr, &PlanOptions::range_guard, nullptr, true, true, false},
    {"fuse_front", nullptr, &PlanOptions::fuse_front, nullptr, true, true, false},   // (0: stem -> conv_split -> conv_dma stride 2, three kernels)
    {"fuse_pairs", nullptr, &PlanOptions::fuse_pairs, nullptr, true, true, false},
    {"share_s", nullptr, &PlanOptions::share_s, nullptr, true, true, false},
    {"fold_final", nullptr, &PlanOptions::fold_final, nullptr, true, true, false},
    {"fold_down", nullptr, &PlanOptions::fold_down, nullptr, true, true, false},
    {"fold_lo", nullptr, &PlanOptions::fold_lo, nullptr, true, true, false},
    {"profile_tag_ops", nullptr, &PlanOptions::profile_tag_ops, nullptr, true, true, false},
    {"table_batch", nullptr, &PlanOptions::table_batch, nullptr, false, true, true},
    {"normalize_ranges", nullptr, &PlanOptions::normalize_ranges, nullptr, true, false, false},
    {"train_side_stream", nullptr, nullptr, &g_opt_train_side, true, false, false},
    {"wgrad_taps", nullptr, nullptr, &g_opt_wgrad_taps, true, false, false},
    {"train_forward_s4", nullptr, nullptr, &g_opt_train_s4, true, false, false},
    {"train_blocked_sum", nullptr, nullptr, &g_opt_train_kacc, true, false, false},
    {"train_table_batch", nullptr, nullptr, &g_opt_train_table_batch, true, false, true},
    {"upsample_bwd_two_pass", nullptr, nullptr, &g_opt_up_two_pass, true, false, false},
};

// plan == nullptr: the process-wide value
int set_option(const char *who, PlanOptions *plan, const char *name, int value) {
    for (const Option &o : kOptions) {
        if (strcmp(name, o.name) != 0 && !(o.alias && !strcmp(name, o.alias))) continue;
        if (!(plan ? o.per_plan : o.process)) break;
        if (o.clamp0 && value < 0) value = 0;
        *(o.member ? &((plan ? *plan : g_plan_opt).*o.member) : o.global) = value;
        return PF_OK;
    }
    return fail(PF_EINVAL, "%s: unknown option '%s'", who, name);
}

}  // namespace

extern "C" int pf_set_option(const char *name, int value) {
    if (!name) return fail(PF_EINVAL, "pf_set_option: null name");
    return set_option("pf_set_option", nullptr, name, value);
}

extern "C" int pf_hardnet_plan_set_option(pf_plan *p, const char *name, int value) {
    if (!p || !name) return fail(PF_EINVAL, "pf_hardnet_plan_set_option: null argument");
    return set_option("pf_hardnet_plan_set_option", &p->opt, name, value);
}

// P = 3x3 conv of ONE range S, C = 3x3 conv whose first range is exactly P's output and whose second range is exactly S
// (hardnet.py:177-194: the links of an even layer start with the odd layer in front of it and contain that layer's input)
bool pf::is_conv_pair(const NetTable &t, size_t i) {
    if (i + 1 >= t.ops.size()) return false;
    const BlobOp &P = t.ops[i], &C = t.ops[i + 1];
    if (P.kind != OP_CONV || C.kind != OP_CONV || P.k != 3 || C.k != 3 || P.stride != 1 || C.stride != 1) return false;
    if (P.n_src != 1 || C.n_src < 2 || (P.dst_choff & 1) || (C.dst_choff & 1)) return false;
    if (C.src[0].tensor != P.dst || C.src[0].choff != P.dst_choff || C.src[0].ch != P.cout) return false;
    if (C.src[1].tensor != P.src[0].tensor || C.src[1].choff != P.src[0].choff || C.src[1].ch != P.src[0].ch) return false;
    for (uint32_t j = 0; j < C.n_src; ++j)
        if (C.src[j].choff & 1) return false;
    return conv_pair_supports((int)C.cout, (int)P.cout);
}

// L = op i, a 3x3 stride-1 conv of the form's two or three cout tiles; R = the 1x1 stride-1 conv behind it whose range ends with L's
// slice: op i + 1 and its single range, or (FoldDesc::up) op i + 2 behind the upsample op i + 1 of that range, whose whole output is the
// first of R's two ranges and read by nothing else.  The slice and the range start on a 4-channel boundary, the range's other channels
// (in front of the slice) are at most 8 groups - one K = 32 chunk of the fold forms - and every one of them was written by an earlier
// op.  What the form adds (kFolds): R's ReLU (up: R's own belongs to its other half) and cout tiles; tail: R is the only op that reads
// the slice, which is never stored; down: op i + 2 is the 2x2 average pool of R's output, its only reader, and other ops may read the
// slice: it is stored.  (The formats of L's and R's destinations and which kernels they run on are known to the schedule only:
// hardnet_plan.hip.)
bool pf::is_conv_fold(const NetTable &t, size_t i, FoldForm form) {
    const FoldDesc &f = kFolds[form];
    const size_t ri = i + f.r_at();
    if (ri + (f.pool ? 1 : 0) >= t.ops.size()) return false;
    const BlobOp &L = t.ops[i], &R = t.ops[ri];
    if (L.kind != OP_CONV || R.kind != OP_CONV || L.k != 3 || L.stride != 1 || R.k != 1 || R.stride != 1 || R.n_src != (f.up ? 2u : 1u)) return false;
    if (!f.up && (R.relu != 0) != f.r_relu) return false;
    if (L.cout <= 16u * (f.l_tiles - 1) || L.cout > 16u * f.l_tiles || R.cout > 16u * f.r_tiles) return false;
    if (f.pool) {
        const BlobOp &P = t.ops[i + 2];
        if (P.kind != OP_POOL || P.src[0].tensor != R.dst || R.dst_choff != 0 || R.cout != t.tensors[R.dst].channels) return false;
    }
    if (f.up) {
        const BlobOp &U = t.ops[i + 1];
        if (U.kind != OP_UPSAMPLE || R.src[0].tensor != U.dst || R.src[0].choff != 0 || R.src[0].ch != t.tensors[U.dst].channels || U.src[0].ch != R.src[0].ch)
            return false;
    }
    for (uint32_t j = 0; j < L.n_src; ++j)
        if (L.src[j].choff & 1) return false;
    const BlobSrc &rs = t.ops[i + 1].src[0];   // the range: R's, or the upsample's
    const uint32_t d0 = L.dst_choff, d1 = L.dst_choff + L.cout;
    if (rs.tensor != L.dst || (rs.choff & 3) || (d0 & 3) || rs.choff > d0 || rs.choff + rs.ch != d1 || d0 - rs.choff > 32) return false;
    std::vector<uint8_t> written(t.tensors[L.dst].channels, 0);
    for (size_t j = 0; j < t.ops.size(); ++j) {
        const BlobOp &o = t.ops[j];
        if (j < i && (o.kind == OP_CONV || o.kind == OP_STEM) && o.dst == L.dst)
            for (uint32_t c = o.dst_choff; c < o.dst_choff + o.cout && c < written.size(); ++c) written[c] = 1;
        for (uint32_t s = 0; s < o.n_src; ++s) {
            const BlobSrc &os = o.src[s];
            if (!f.other_readers && j != i + 1 && os.tensor == L.dst && os.choff < d1 && os.choff + os.ch > d0) return false;   // another reader of the slice
            if (f.pool && j != i + 2 && os.tensor == R.dst) return false;   // the pool is the only reader of R's output
            if (f.up && j != ri && os.tensor == t.ops[i + 1].dst) return false;   // R is the only reader of the upsample's
        }
    }
    for (uint32_t c = rs.choff; c < d0; ++c)
        if (!written[c]) return false;
    return true;
}

// Cityscapes id -> trainId (public label table; ids outside 0..33 -> 0, like the zeros_like init of
// export_cityscapes_segmentation_results.py:34-38)
static void fill_lut(uint8_t *lut) {
    memset(lut, 0, 256);
    for (int i = 0; i < 34; ++i) lut[i] = 255;
    const int ids[19] = {7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33};
    for (int t = 0; t < 19; ++t) lut[ids[t]] = (uint8_t)t;
}

// Range normalisation (conv_mfma.h, "low side"): a static range propagation over the op table.  est[t][c] = expected magnitude
// (rms-like) of channel c of tensor t in the ORIGINAL units: 1 for dense inputs (sqrt(1/n_cls) for the one-hot channels of the
// fused stem), sqrt(sum_k |w_ok|^2 est_k^2 + b_o^2) behind a conv (uncorrelated-inputs model), / sqrt(2) behind a ReLU, copied
// through pool / upsample.  Channel c is then STORED multiplied by s = 2^round(log2(kRangeTarget / est)): the producer's
// weight row and bias are multiplied by s, every consumer's weight column divided by it - powers of two, so the network
// computes bit-identical fp32 products; only where the fp16 pair's subnormal floor (2^-25 absolute) and its ceiling (65504)
// fall relative to the data changes.  A checkpoint re-parameterised across a BatchNorm (gamma * alpha, next weights / alpha)
// gets s / alpha and stores the same values.  Channels of tensors no convolution reads (network outputs, the head's input)
// keep s = 1.  The guarantee itself is the run-time guard (PF_STATUS_RANGE / PF_STATUS_RANGE_LOW); this only decides how
// often it fires.
static void normalize_ranges(pf_plan *p, std::vector<float> &w) {
    const size_t nT = p->net.tensors.size();
    p->chan_scale.assign(nT, std::vector<float>());
    std::vector<std::vector<double>> est(nT);
    for (size_t t = 0; t < nT; ++t) {
        p->chan_scale[t].assign(p->net.tensors[t].channels, 1.0f);
        est[t].assign(p->net.tensors[t].channels, 1.0);
    }
    // feeds_conv: backwards over the table (ops are in topological order)
    p->feeds_conv.assign(nT, 0);
    for (size_t i = p->net.ops.size(); i-- > 0;) {
        const BlobOp &o = p->net.ops[i];
        if (o.kind == OP_STEM || o.kind == OP_CONV)
            for (uint32_t j = 0; j < o.n_src; ++j) p->feeds_conv[o.src[j].tensor] = 1;
        else if ((o.kind == OP_POOL || o.kind == OP_UPSAMPLE) && p->feeds_conv[o.dst])
            p->feeds_conv[o.src[0].tensor] = 1;
    }
    // pinned to s = 1: read by the head, by nobody (outputs tapped by the caller), or the network input
    std::vector<uint8_t> pinned(nT, 0), read(nT, 0);
    for (const BlobOp &o : p->net.ops) {
        for (uint32_t j = 0; j < (o.kind == OP_UPSAMPLE ? 1u : o.n_src); ++j) read[o.src[j].tensor] = 1;
        if (o.kind == OP_HEAD) pinned[o.src[0].tensor] = 1;
    }
    for (size_t t = 0; t < nT; ++t) pinned[t] = pinned[t] || !read[t] || !p->feeds_conv[t];
    if (p->net.ops.empty()) return;
    const uint32_t input = p->net.ops[0].src[0].tensor;
    pinned[input] = 1;
    if (p->net.ops[0].kind == OP_STEM && p->net.hdr.n_cls > 0) {   // fused stem: T * n_cls one-hot channels, then T depth channels
        const uint32_t C = p->net.tensors[input].channels, T = C / (p->net.hdr.n_cls + 1);
        if (T * (p->net.hdr.n_cls + 1) == C)
            for (uint32_t c = 0; c < T * p->net.hdr.n_cls; ++c) est[input][c] = std::sqrt(1.0 / p->net.hdr.n_cls);
    }
    // pool / upsample outputs inherit their source's scale: they are pinned iff ... their source is; a pinned destination of
    // such an op pins the source channel too (the scale must be the same on both sides), so walk backwards first
    for (size_t i = p->net.ops.size(); i-- > 0;) {
        const BlobOp &o = p->net.ops[i];
        if ((o.kind == OP_POOL || o.kind == OP_UPSAMPLE) && pinned[o.dst]) pinned[o.src[0].tensor] = 1;
    }
    for (const BlobOp &o : p->net.ops) {
        if (o.kind == OP_POOL || o.kind == OP_UPSAMPLE) {
            for (uint32_t c = 0; c < o.src[0].ch; ++c) {
                p->chan_scale[o.dst][o.dst_choff + c] = p->chan_scale[o.src[0].tensor][o.src[0].choff + c];
                est[o.dst][o.dst_choff + c] = est[o.src[0].tensor][o.src[0].choff + c];
            }
            continue;
        }
        if (o.kind != OP_STEM && o.kind != OP_CONV) continue;
        const size_t kk = (size_t)o.k * o.k;
        // input channel k of the conv -> (estimate, stored scale)
        std::vector<double> e_in(o.cin);
        std::vector<float> s_in(o.cin);
        uint32_t k0 = 0;
        for (uint32_t j = 0; j < o.n_src; ++j)
            for (uint32_t c = 0; c < o.src[j].ch; ++c, ++k0) {
                e_in[k0] = est[o.src[j].tensor][o.src[j].choff + c];
                s_in[k0] = p->chan_scale[o.src[j].tensor][o.src[j].choff + c];
            }
        for (uint32_t co = 0; co < o.cout; ++co) {
            float *wr = w.data() + o.w_off + (size_t)co * o.cin * kk;
            float &b = w[o.b_off + co];
            double var = (double)b * b;
            for (uint32_t k = 0; k < o.cin; ++k) {
                double ss = 0;
                for (size_t q = 0; q < kk; ++q) ss += (double)wr[k * kk + q] * wr[k * kk + q];
                var += ss * e_in[k] * e_in[k];
            }
            double e = std::sqrt(var);
            if (o.relu) e *= 0.70710678118654752;
            float s_out = 1.0f;
            if (p->opt.normalize_ranges && !pinned[o.dst] && e > 0 && std::isfinite(e)) {
                int ex = (int)std::lround(std::log2((double)kRangeTarget / e));
                ex = ex < -60 ? -60 : (ex > 60 ? 60 : ex);
                s_out = std::ldexp(1.0f, ex);
            }
            for (uint32_t k = 0; k < o.cin; ++k) {
                const float f = s_out / s_in[k];   // a power of two
                if (f != 1.0f)
                    for (size_t q = 0; q < kk; ++q) wr[k * kk + q] *= f;
            }
            b *= s_out;
            p->chan_scale[o.dst][o.dst_choff + co] = s_out;
            est[o.dst][o.dst_choff + co] = e;
        }
    }
}

namespace {

// the host image of dev_weights: regions handed out in order, each at a multiple of `align` floats, padding zero-filled
struct Arena {
    std::vector<float> &f;
    size_t take(size_t n_floats, size_t align = 1) {
        f.resize(align_up(f.size(), align), 0.f);
        f.resize(f.size() + n_floats);
        return f.size() - n_floats;
    }
    float *at(size_t off) { return f.data() + off; }
};

// The packers: one per kernel family, each given the op, its folded weights w (OIHW; ws = scaled by the conv's 2^k), the
// channels of its input ranges and the arena, each filling in its own fields of the ConvPlan
void pack_generic(const BlobOp &o, const float *w, const float *bias, Arena &a, ConvPlan &c) {
    c.tiling = choose_tiling((int)o.k, (int)o.stride, (int)o.cin, (int)o.cout, 0);
    c.wpk_off = a.take(c.tiling.packed_floats());
    pack_conv_weights(w, (int)o.cin, (int)o.cout, c.tiling, a.at(c.wpk_off));
    c.bias_off = a.take((size_t)c.tiling.cout_blocks * c.tiling.nt * 16);
    memcpy(a.at(c.bias_off), bias, o.cout * sizeof(float));
}

void pack_dma(const BlobOp &o, const float *w, const int *src_ch, Arena &a, ConvPlan &c) {
    const int kc = dma_kc((int)o.k, (int)o.stride);
    c.tiled_chunks = range_chunks(src_ch, (int)o.n_src, kc);
    c.tiled_off = a.take(tiled_packed_floats(src_ch, (int)o.n_src, (int)o.cout, (int)o.k, (int)o.stride));
    pack_conv_weights_tiled(w, (int)o.cin, (int)o.cout, (int)o.k, kc, src_ch, (int)o.n_src, a.at(c.tiled_off));
    // trailing couts that may run on the vector ALU beside the MFMA tiles (conv_dma.hip): groups of at most valu_max (beyond
    // that the padded MFMA tile measured faster)
    constexpr int valu_max = 8;
    const int split = (o.k == 3 && o.stride == 1) ? dma_valu_split((int)o.cout) : 0;
    if (split > 0 && split <= valu_max) {
        c.rem_count = split;
        c.rem_off = a.take(rem_packed_floats(src_ch, (int)o.n_src, split, 3, kc), 4);
        pack_conv_weights_rem(w, (int)o.cin, (int)o.cout, split, 3, kc, src_ch, (int)o.n_src, a.at(c.rem_off));
    }
}

// w * 2^k, the exact scaling whose fp16 terms the split / S4 / pair / front packings hold (k per conv: conv_mfma.h); returns 2^k
float scale_weights(const float *w, size_t n, std::vector<float> &ws) {
    const float sc = split_weight_scale(w, n);
    ws.resize(n);
    for (size_t q = 0; q < n; ++q) ws[q] = w[q] * sc;
    return sc;
}

void pack_split(const BlobOp &o, const float *ws, const int *src_ch, Arena &a, ConvPlan &c) {   // stride 1: 3x3 or 1x1
    if (o.k == 3) {
        c.split_chunks = range_chunks(src_ch, (int)o.n_src, 8);
        c.split_off = a.take(split_packed_floats(src_ch, (int)o.n_src, (int)o.cout), 16);
        pack_conv_weights_split(ws, (int)o.cin, (int)o.cout, src_ch, (int)o.n_src, a.at(c.split_off));
    } else {
        c.split_chunks = range_chunks(src_ch, (int)o.n_src, 32);
        c.split_off = a.take(split1_packed_floats(src_ch, (int)o.n_src, (int)o.cout), 16);
        pack_conv_weights_split1(ws, (int)o.cin, (int)o.cout, src_ch, (int)o.n_src, a.at(c.split_off));
    }
}

void pack_s4(const BlobOp &o, const float *ws, Arena &a, ConvPlan &c) {   // stride 1; none if a range starts at an odd channel
    for (uint32_t j = 0; j < o.n_src; ++j)
        if (o.src[j].choff & 1) return;
    const KOrder ko = order_plain(o.src, (int)o.n_src);
    c.s4_pad = o.k == 1 && o.n_src == 2;
    c.s4_rounds = s4_rounds(ko, (int)o.k, c.s4_pad);
    c.s4_off = a.take(s4_packed_floats(ko, (int)o.cout, (int)o.k, c.s4_pad), 16);
    pack_conv_weights_s4(ws, (int)o.cin, (int)o.cout, (int)o.k, ko, c.s4_pad, a.at(c.s4_off));
}

// conv_pair.hip: o is the consumer C of a pair, P its producer (the op before it).  C's weights in the pair's K order (order_pair), every
// range padded to whole rounds; P's weights (wP: unscaled) as two-instruction rounds + a ninth-tap stream, scaled by P's own 2^k
void pack_pair(const BlobOp &P, const float *wP, const BlobOp &o, const float *ws, Arena &a, ConvPlan &c) {
    const KOrder ko = order_pair(o.src, (int)o.n_src);
    c.pair_rounds = s4_rounds(ko, 3, 1);
    c.pair_c_off = a.take(s4_packed_floats(ko, (int)o.cout, 3, 1), 16);
    std::vector<float> wp;
    scale_weights(wP, (size_t)P.cout * P.cin * 9, wp);
    c.pair_merged = conv_pair_merged_supports((int)o.cout, (int)P.cout);
    if (c.pair_merged) {
        // P's couts ride in the rows C's last cout tile pads with zeros (from the next multiple of four on), over the columns of
        // S: C's matrix instructions over S then produce P at the tile's own pixels for nothing.  Harmless for the plain kernel
        // (its epilogue never looks at those rows)
        const int nt = ((int)o.cout + 15) / 16, row0 = ((int)o.cout + 3) / 4 * 4, cS = ko.r[0].cstart;   // (S leads the order)
        std::vector<float> waug((size_t)nt * 16 * o.cin * 9, 0.f);
        std::copy(ws, ws + (size_t)o.cout * o.cin * 9, waug.begin());
        for (int pc = 0; pc < (int)P.cout; ++pc)
            for (int ci = 0; ci < (int)P.cin; ++ci)
                for (int t = 0; t < 9; ++t) waug[((size_t)(row0 + pc) * o.cin + cS + ci) * 9 + t] = wp[((size_t)pc * P.cin + ci) * 9 + t];
        pack_conv_weights_s4(waug.data(), (int)o.cin, nt * 16, 3, ko, 1, a.at(c.pair_c_off));
    } else {
        pack_conv_weights_s4(ws, (int)o.cin, (int)o.cout, 3, ko, 1, a.at(c.pair_c_off));
    }
    const S4Range rs{(int)P.src[0].choff, (int)P.src[0].ch};
    c.pair_two_off = a.take(pair_p_two_floats(rs, (int)P.cout), 16);
    c.pair_nine_off = a.take(pair_p_nine_floats(rs, (int)P.cout), 16);
    pack_conv_weights_pair_p(wp.data(), (int)P.cin, (int)P.cout, rs, a.at(c.pair_two_off), a.at(c.pair_nine_off));
}

// conv_s4.hip share / add: o is the consumer C of a pair, P its producer.  The share launch's matrix over S: P's rows (scaled by P's own
// 2^k), zero rows up to share_row0, C's rows restricted to the columns of S (C's 2^k); the add launch's: C over [P's output, others..] (order_add)
void pack_share(const BlobOp &P, const float *wP, const BlobOp &o, const float *ws, Arena &a, ConvPlan &c) {
    const int row0 = share_row0((int)P.cout), rows = row0 + (int)o.cout, cS = (int)o.src[0].ch;
    std::vector<float> wp, wa((size_t)rows * P.cin * 9, 0.f);
    scale_weights(wP, (size_t)P.cout * P.cin * 9, wp);
    std::copy(wp.begin(), wp.end(), wa.begin());
    for (int co = 0; co < (int)o.cout; ++co)
        for (int ci = 0; ci < (int)P.cin; ++ci)
            for (int t = 0; t < 9; ++t) wa[((size_t)(row0 + co) * P.cin + ci) * 9 + t] = ws[((size_t)co * o.cin + cS + ci) * 9 + t];
    const KOrder ko_s = order_plain(P.src, 1), ko_b = order_add(o.src, (int)o.n_src);
    c.share_a_tiles = (rows + 15) / 16;
    c.share_a_off = a.take(s4_packed_floats(ko_s, rows, 3, 0), 16);
    pack_conv_weights_s4(wa.data(), (int)P.cin, rows, 3, ko_s, 0, a.at(c.share_a_off));
    c.share_b_rounds = s4_rounds(ko_b, 3, 0);
    c.share_b_off = a.take(s4_packed_floats(ko_b, (int)o.cout, 3, 0), 16);
    pack_conv_weights_s4(ws, (int)o.cin, (int)o.cout, 3, ko_b, 0, a.at(c.share_b_off));
}

// conv_s4.hip folds: o is the 3x3 conv, R the 1x1 conv behind it, `range` the range that ends with o's slice - R's, or the upsample's
// between them, whose channels are R's first (is_conv_fold) -, wr = R's weights times R's 2^k (the power-of-two scale of every source
// channel folded in by normalize_ranges, as for R's own packings).  Into the form's region of the plan, cout tile by cout tile
void pack_fold(FoldForm form, const BlobOp &o, const BlobOp &R, const BlobSrc &range, const float *wr, Arena region, ConvPlan &c) {
    const FoldDesc &f = kFolds[form];
    c.fold_off[form] = region.take(fold_packed_floats(f.r_tiles, f.chunks()), 16);
    pack_conv_weights_fold(wr, (int)R.cin, (int)R.cout, order_tail(range, (int)o.dst_choff, (int)o.cout), f.r_tiles, region.at(c.fold_off[form]), f.chunks());
}

void pack_front(const BlobOp &o, const float *ws, Arena &a, ConvPlan &c) {   // 3x3 stride 2, one range
    const KOrder ko = order_plain(o.src, 1);
    c.front_off = a.take(s4_packed_floats(ko, (int)o.cout, 3, 0), 16);
    pack_conv_weights_s4(ws, (int)o.cin, (int)o.cout, 3, ko, 0, a.at(c.front_off));
}

void pack_wave(const BlobOp &o, const float *w, const int *src_ch, Arena &a, ConvPlan &c) {   // stride 1
    c.wave_chunks = range_chunks(src_ch, (int)o.n_src, wave_kc((int)o.k));
    c.wave_off = a.take(wave_packed_floats(src_ch, (int)o.n_src, (int)o.cout, (int)o.k));
    pack_conv_weights_wave(w, (int)o.cin, (int)o.cout, (int)o.k, src_ch, (int)o.n_src, a.at(c.wave_off));
}

void pack_stem(const BlobOp &o, const float *w, int n_cls, Arena &a, ConvPlan &c) {
    const int ks2 = (int)(o.k * o.k);
    c.raw_off = a.take((size_t)o.cout * o.cin * ks2);
    memcpy(a.at(c.raw_off), w, (size_t)o.cout * o.cin * ks2 * sizeof(float));
    // depth channels are the last T of the T*(n_cls+1) inputs (bg_model.py:68-69)
    const int T = (int)o.cin / (n_cls + 1);
    if (T < 1 || (uint32_t)(T * (n_cls + 1)) != o.cin || o.cout != 16) return;
    c.dep_off = a.take((size_t)ks2 * T * 16, 16);
    float *q = a.at(c.dep_off);
    for (int tap = 0; tap < ks2; ++tap)
        for (int t = 0; t < T; ++t)
            for (int co = 0; co < 16; ++co) *q++ = w[((size_t)co * o.cin + T * n_cls + t) * ks2 + tap];
    c.oh_off = a.take((size_t)ks2 * T * (n_cls + 1) * 16, 16);
    q = a.at(c.oh_off);
    for (int tap = 0; tap < ks2; ++tap)
        for (int t = 0; t < T; ++t)
            for (int r = 0; r <= n_cls; ++r)
                for (int co = 0; co < 16; ++co) *q++ = r < n_cls ? w[((size_t)co * o.cin + t * n_cls + r) * ks2 + tap] : 0.f;
}

// Host only: every packing of every convolution of the (range-normalised) folded weights, and the reciprocals of the plan's
// channel scales, into `host` - the image of dev_weights, whose first 64 floats are the zero page
int build_plan_weights(pf_plan &p, const float *wts, std::vector<float> &host) {
    host.assign(64, 0.f);
    Arena a{host};
    for (pf_plan::FoldRegion &r : p.fold) r.host.assign(64, 0.f);
    const std::vector<BlobOp> &ops = p.net.ops;
    p.conv.assign(ops.size(), ConvPlan());
    for (size_t i = 0; i < ops.size(); ++i) {
        const BlobOp &o = ops[i];
        if (o.kind != OP_STEM && o.kind != OP_CONV) continue;
        if (o.k == 1 && o.stride != 1) return fail(PF_EUNSUPPORTED, "1x1 conv with stride %u", o.stride);
        ConvPlan &c = p.conv[i];
        const float *w = wts + o.w_off, *ws = w;
        int src_ch[kConvMaxSrc];
        for (uint32_t j = 0; j < o.n_src; ++j) src_ch[j] = (int)o.src[j].ch;
        pack_generic(o, w, wts + o.b_off, a, c);
        pack_dma(o, w, src_ch, a, c);
        std::vector<float> wsc;
        if (o.stride == 1 || o.n_src == 1) {
            c.split_acc_scale = 1.0f / scale_weights(w, (size_t)o.cout * o.cin * o.k * o.k, wsc);
            ws = wsc.data();
        }
        if (o.stride == 1) pack_split(o, ws, src_ch, a, c);
        if (o.stride == 1 && o.kind == OP_CONV) pack_s4(o, ws, a, c);
        if (i > 0 && is_conv_pair(p.net, i - 1)) pack_pair(ops[i - 1], wts + ops[i - 1].w_off, o, ws, a, c);
        if (i > 0 && p.opt.share_s && is_conv_pair(p.net, i - 1)) pack_share(ops[i - 1], wts + ops[i - 1].w_off, o, ws, a, c);
        if (o.k == 3 && o.stride == 2 && o.kind == OP_CONV && o.n_src == 1 && (o.src[0].choff & 3) == 0 && o.cout <= 32) pack_front(o, ws, a, c);
        for (int f = 0; f < kFoldForms; ++f) {   // (o = the reader)
            const size_t back = kFolds[f].r_at();
            if (i >= back && p.opt.*kFolds[f].option && is_conv_fold(p.net, i - back, (FoldForm)f))
                pack_fold((FoldForm)f, ops[i - back], o, ops[i - back + 1].src[0], ws, Arena{p.fold[f].host}, p.conv[i - back]);
        }
        if (o.stride == 1) pack_wave(o, w, src_ch, a, c);
        if (o.kind == OP_STEM) pack_stem(o, w, (int)p.net.hdr.n_cls, a, c);
        a.take(0, 64);
    }
    p.inv_scale_off.assign(p.net.tensors.size(), 0);
    for (size_t t = 0; t < p.net.tensors.size(); ++t) {
        bool any = false;
        for (float v : p.chan_scale[t]) any = any || v != 1.0f;
        if (!any) continue;
        p.inv_scale_off[t] = a.take(p.chan_scale[t].size());
        for (size_t ch = 0; ch < p.chan_scale[t].size(); ++ch) host[p.inv_scale_off[t] + ch] = 1.0f / p.chan_scale[t][ch];   // exact: powers of two
        a.take(0, 64);
    }
    for (pf_plan::FoldRegion &r : p.fold)
        if (r.host.size() == 64) r.host.clear();   // no op has the form
    return PF_OK;
}

// what only the inference plan asks of the table: every convolution's cin, destination range, kernel and weights inside the blob
// (n_w floats); a pool / upsample range that fits its destination
int check_plan_ops(const NetTable &t, size_t n_w) {
    for (size_t i = 0; i < t.ops.size(); ++i) {
        const BlobOp &o = t.ops[i];
        uint32_t cin = 0;
        for (uint32_t j = 0; j < o.n_src; ++j) cin += o.src[j].ch;
        bool ok = true;
        if (o.kind == OP_STEM || o.kind == OP_CONV)
            ok = cin == o.cin && o.dst_choff + o.cout <= t.tensors[o.dst].channels && (o.k == 1 || o.k == 3) &&
                 (o.stride == 1 || o.stride == 2) && o.w_off + (uint64_t)o.cout * o.cin * o.k * o.k <= n_w && o.b_off + o.cout <= n_w;
        if (o.kind == OP_POOL || o.kind == OP_UPSAMPLE) ok = o.src[0].ch <= t.tensors[o.dst].channels;
        if (!ok) return fail(PF_EBLOB, "op %zu is inconsistent with the tensor table", i);
    }
    return PF_OK;
}

void count_readers(pf_plan &p) {
    p.readers.assign(p.net.tensors.size(), 0);
    for (const BlobOp &o : p.net.ops)
        for (uint32_t j = 0; j < o.n_src; ++j) p.readers[o.src[j].tensor]++;
}

}  // namespace

extern "C" int pf_hardnet_plan_create(const void *blob, size_t bytes, int in_ch, int n_cls, pf_plan **out) {
    if (!blob || !out) return fail(PF_EINVAL, "pf_hardnet_plan_create: null argument");
    pf_plan *p = new pf_plan();
    p->opt = g_plan_opt;
    int rc = parse_net_table(blob, bytes, in_ch, n_cls, p->net);
    // (ranked above a malformed op of the table, which parse_net_table reports with the table filled in)
    if ((int)p->net.ops.size() >= kMaxSlots - 1)
        rc = fail(PF_EUNSUPPORTED, "op table of %zu ops: the status block has %d per-op words", p->net.ops.size(), kMaxSlots - 1);
    const size_t n_w = rc ? 0 : (bytes - p->net.hdr.weights_off) / sizeof(float);
    if (!rc) rc = check_plan_ops(p->net, n_w);
    std::vector<float> wnorm, host;
    if (!rc) {
        // the folded weights, re-parameterised so that every stored channel has an expected magnitude of kRangeTarget
        const float *w0 = reinterpret_cast<const float *>((const char *)blob + p->net.hdr.weights_off);
        wnorm.assign(w0, w0 + n_w);
        normalize_ranges(p, wnorm);
        rc = build_plan_weights(*p, wnorm.data(), host);
    }
    if (rc) {
        delete p;
        return rc;
    }
    count_readers(*p);
    p->dev_floats = host.size();
    uint8_t lut[256];
    fill_lut(lut);
    hipError_t e = hipMalloc((void **)&p->dev_weights, (host.size() + 64) * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&p->dev_lut, 256);
    if (e == hipSuccess) e = hipMemcpy(p->dev_weights, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->dev_lut, lut, 256, hipMemcpyHostToDevice);
    for (pf_plan::FoldRegion &r : p->fold) {
        if (e == hipSuccess && !r.host.empty()) e = hipMalloc((void **)&r.dev, r.host.size() * sizeof(float));
        if (e == hipSuccess && r.dev) e = hipMemcpy(r.dev, r.host.data(), r.host.size() * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        pf_hardnet_plan_destroy(p);
        return fail(PF_EHIP, "plan upload: %s", hipGetErrorString(e));
    }
    *out = p;
    return PF_OK;
}

// Host only, no device involved (tests): the plan this blob would give now under the process-wide options, with everything but
// the uploads (`host` = its weight arena; the fold regions stay in pf_plan::fold[].host)
int pf::debug_plan(const char *who, const void *blob, size_t bytes, int in_ch, int n_cls, const size_t *n_floats, pf_plan &p, std::vector<float> &host) {
    if (!blob || !n_floats) return fail(PF_EINVAL, "%s: null argument", who);
    p.opt = g_plan_opt;
    int rc = parse_net_table(blob, bytes, in_ch, n_cls, p.net);
    const size_t n_w = rc ? 0 : (bytes - p.net.hdr.weights_off) / sizeof(float);
    if (!rc) rc = check_plan_ops(p.net, n_w);
    if (rc) return rc;
    const float *w0 = reinterpret_cast<const float *>((const char *)blob + p.net.hdr.weights_off);
    std::vector<float> wnorm(w0, w0 + n_w);
    normalize_ranges(&p, wnorm);
    count_readers(p);
    return build_plan_weights(p, wnorm.data(), host);
}

// the weight arena that plan would upload (every packing of every convolution), and per op of the table six numbers: offset (floats)
// and rounds of its packed-pair packing, offset and cout tiles of the share launch's, offset and rounds of the add launch's (0 = the op
// has none)
extern "C" int pf_debug_plan_arena(const void *blob, size_t bytes, int in_ch, int n_cls, float *out, size_t cap, size_t *n_floats,
                                   long long *table, int table_ops) {
    pf_plan p;
    std::vector<float> host;
    if (int rc = debug_plan("pf_debug_plan_arena", blob, bytes, in_ch, n_cls, n_floats, p, host)) return rc;
    *n_floats = host.size();
    if (out && cap >= host.size()) memcpy(out, host.data(), host.size() * sizeof(float));
    for (int i = 0; table && i < table_ops && i < (int)p.conv.size(); ++i) {
        const ConvPlan &c = p.conv[i];
        const long long row[6] = {(long long)c.s4_off, c.s4_rounds, (long long)c.share_a_off, c.share_a_tiles, (long long)c.share_b_off, c.share_b_rounds};
        memcpy(table + 6 * i, row, sizeof(row));
    }
    return PF_OK;
}

// a fold form's region of that plan - tail: option "fold_final", down and down3: "fold_down", lo: "fold_lo" - (its first 64 floats are
// zeros) and per op of the table its offset into it (0 = the op has no such packing)
static int debug_plan_fold(const char *who, FoldForm form, const void *blob, size_t bytes, int in_ch, int n_cls, float *out, size_t cap, size_t *n_floats,
                           long long *table, int table_ops) {
    pf_plan p;
    std::vector<float> host;
    if (int rc = debug_plan(who, blob, bytes, in_ch, n_cls, n_floats, p, host)) return rc;
    const std::vector<float> &region = p.fold[form].host;
    *n_floats = region.size();
    if (out && cap >= region.size() && !region.empty()) memcpy(out, region.data(), region.size() * sizeof(float));
    for (int i = 0; table && i < table_ops && i < (int)p.conv.size(); ++i) table[i] = (long long)p.conv[i].fold_off[form];
    return PF_OK;
}
extern "C" int pf_debug_plan_tail(const void *blob, size_t bytes, int in_ch, int n_cls, float *out, size_t cap, size_t *n_floats,
                                  long long *table, int table_ops) {
    return debug_plan_fold("pf_debug_plan_tail", FOLD_TAIL, blob, bytes, in_ch, n_cls, out, cap, n_floats, table, table_ops);
}
extern "C" int pf_debug_plan_down(const void *blob, size_t bytes, int in_ch, int n_cls, float *out, size_t cap, size_t *n_floats,
                                  long long *table, int table_ops) {
    return debug_plan_fold("pf_debug_plan_down", FOLD_DOWN, blob, bytes, in_ch, n_cls, out, cap, n_floats, table, table_ops);
}

// form: 2 = down3, 3 = lo (the forms of three-tile producers)
extern "C" int pf_debug_plan_wide(int form, const void *blob, size_t bytes, int in_ch, int n_cls, float *out, size_t cap, size_t *n_floats,
                                  long long *table, int table_ops) {
    if (form != FOLD_DOWN3 && form != FOLD_LO) return fail(PF_EINVAL, "pf_debug_plan_wide: form %d", form);
    return debug_plan_fold("pf_debug_plan_wide", (FoldForm)form, blob, bytes, in_ch, n_cls, out, cap, n_floats, table, table_ops);
}

extern "C" void pf_hardnet_plan_destroy(pf_plan *p) {
    if (!p) return;
    if (p->dev_weights) (void)hipFree(p->dev_weights);
    if (p->dev_lut) (void)hipFree(p->dev_lut);
    for (pf_plan::FoldRegion &r : p->fold)
        if (r.dev) (void)hipFree(r.dev);
    delete p;
}
