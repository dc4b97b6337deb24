// fg forecaster, host only (no HIP call, no kernel): the tensor and GEMM tables, the layouts of the packed weights and of the workspace,
// and build_fg_schedule - which buffer every launch of a forward reads and writes (the h0 ring of max(T_in, 2) slots, the h1
// ping-pong, c in place) and whether a 3x3 GEMM has a pair form, settled before anything is enqueued.  pf_debug_fg_schedule hands the
// tables to tests without a device.
#include <algorithm>
#include <cstring>

#include "fg_net.h"

namespace pf {
namespace fg {

const long long kSize[NTENSOR] = {
    OD, OD, 2, 2, 8, 8,
    3 * HID * 80, 3 * HID * HID, 3 * HID, 3 * HID, 3 * HID * 79, 3 * HID * HID, 3 * HID, 3 * HID,
    HID * HID, HID, TR * HID, TR, HID * HID, HID, TR * HID, TR, TF * HID, TF,
    ICC * C, ICC, IFH * ICC * HW, IFH,
    4LL * C * 528 * 9, 4 * C, 4LL * C * 512 * 9, 4 * C, 4LL * C * 528 * 9, 4 * C, 4LL * C * 512 * 9, 4 * C,
    C * C, C, C * C, C,
    C * C * 9, C, C * C * 9, C, C * C * 9, C, C * C * 9, C, C * C * 4, C, 8 * C, 8};

const GemmDesc kGemm[NGEMM] = {
    {ME0_W, 528, 9, 16, MAP_LSTM}, {ME1_W, 512, 9, 16, MAP_LSTM}, {MD0_W, 528, 9, 16, MAP_LSTM}, {MD1_W, 512, 9, 16, MAP_LSTM},
    {MEO_W, 256, 1, 4, MAP_PLAIN}, {MDO_W, 256, 1, 4, MAP_PLAIN},
    {F1_W, 256, 9, 4, MAP_PLAIN}, {F2_W, 256, 9, 4, MAP_PLAIN}, {F3_W, 256, 9, 4, MAP_PLAIN}, {F4_W, 256, 9, 4, MAP_PLAIN},
    {DC_W, 256, 1, 16, MAP_KMAJOR}};

const int kPairGemm[NPAIR] = {G_ME0, G_ME1, G_MD0, G_MD1, G_F1, G_F2, G_F3, G_F4};

Layout layout() {
    Layout L;
    size_t o = 0;
    for (int i = 0; i < NTENSOR; ++i) {
        L.raw[i] = o;
        o += (size_t)kSize[i];
    }
    L.raw_total = o;
    o = align_up(o, 64);
    for (int g = 0; g < NGEMM; ++g) {
        L.gemm[g] = o;
        o += (size_t)kGemm[g].tiles * 64 * kGemm[g].ctot * kGemm[g].taps;
    }
    L.total = o;
    return L;
}

PairLayout pair_layout(const Layout &L) {
    PairLayout P;
    size_t o = align_up(L.total, 64);
    P.head = o;
    o += 64;
    for (int i = 0; i < NPAIR; ++i) {
        const GemmDesc &d = kGemm[kPairGemm[i]];
        P.gemm[i] = o;
        o += (size_t)d.tiles * ((d.ctot + PKC - 1) / PKC) * PROUND / 2;
    }
    P.total = o;
    return P;
}

Ws ws_layout(int N, int T_in, int flags) {
    Ws w = {};
    const size_t P = (size_t)N * C * HW;
    w.r0 = T_in > 2 ? T_in : 2;
    w.floats[R_STATUS] = (flags & PF_FG_PAIR) ? FG_STATUS_WORDS : 0;
    w.floats[R_INSTF] = (size_t)N * T_in * IFH;
    w.floats[R_INSTD] = (size_t)N * IFH;
    w.floats[R_GRUH] = (size_t)N * HID;
    w.floats[R_TFE] = (size_t)N * T_in * TF;
    w.floats[R_TFD] = (size_t)N * TF;
    w.floats[R_H0] = P * w.r0;
    w.floats[R_H1] = 2 * P;
    w.floats[R_C0] = w.floats[R_C1] = w.floats[R_YA] = w.floats[R_YB] = P;
    w.floats[R_YD] = (size_t)N * C * 784;
    size_t o = 0;
    for (int r = R_STATUS; r < R_FEATS; ++r) {
        w.off[r] = o;
        o = align_up(o + w.floats[r], 64);
    }
    w.total = o * sizeof(float);
    return w;
}

int check_dims(int N, int T_in, int T_out, int flags, int known) {
    if (flags & ~known) return fail(PF_EUNSUPPORTED, "pf_fg: unsupported flags 0x%x (only the shipped fg configuration is built; PF_FG_PAIR is the one switch)", flags);
    if (N < 0 || N > (1 << 20) || T_in < 1 || T_in > 16 || T_out < 1 || T_out > 16)
        return fail(PF_EINVAL, "pf_fg: bad dims N=%d T_in=%d T_out=%d", N, T_in, T_out);
    return 0;
}

int build_fg_schedule(int N, int T_in, int T_out, int flags, std::vector<Step> &steps) {
    if (int rc = check_dims(N, T_in, T_out, flags)) return rc;
    steps.clear();
    steps.reserve(2 * T_in + 5 * T_out + 11);
    const bool pair = flags & PF_FG_PAIR;
    const long long P = (long long)N * C * HW, plane = (long long)C * HW;
    const long long mf_stride = (1 + T_out) * plane;
    const int r0 = T_in > 2 ? T_in : 2;
    int slots = 0, rc = 0;
    auto add = [&](int kind, const char *label) -> Step & {
        Step st = {};
        st.kind = kind, st.label = label, st.gemm = st.pair = st.slot = st.t = -1;
        steps.push_back(st);
        return steps.back();
    };
    // a GEMM launch: x (and vec, h where the cell has them) -> out; a 3x3 one is a pair launch under PF_FG_PAIR
    auto gemm = [&](int g, int epi, Operand x, Operand out, const char *label, const char *pair_label) -> Step & {
        const bool p = pair && kGemm[g].taps == 9;
        Step &st = add(p ? K_PAIR : K_GEMM, p ? pair_label : label);
        st.gemm = g, st.epi = epi, st.x = x, st.nx = C, st.out = out;
        return st;
    };
    auto cell = [&](int g, Operand vec, Operand x, Operand h, Operand out, int c, const char *label, const char *pair_label) {
        Step &st = gemm(g, EPI_LSTM, x, out, label, pair_label);
        st.vec = vec, st.nvec = vec.region ? TF : 0, st.h = h, st.nh = C, st.c = {c, 0, plane};
    };
    if (pair) add(K_STATUS, nullptr);      // last forward's slots judged, word 0 and the slots zeroed (a kernel, never a memset node)
    // ---- encoder: instance features of the T_in input steps (times the step mask), trajectory GRU
    {
        const Operand instf = {R_INSTF, 0, (long long)T_in * IFH};
        Step &f = add(K_INST_FEAT, "pf::fg::inst_feat_kernel");
        f.x = {R_FEATS, 0, T_in * plane}, f.out = instf;
        Step &e = add(K_TRAJ_ENC, "pf::fg::traj_encoder_kernel");
        e.x = instf, e.out = {R_TFE, 0, (long long)T_in * TF}, e.c = {R_GRUH, 0, HID};
    }
    // ---- ConvLSTM encoder, layer-major like convlstm.py:150-166: layer 0 over all steps (h0 slot t), then layer 1 (h1 slot t & 1)
    const Operand none = {R_NONE, 0, plane};
    for (int t = 0; t < T_in; ++t)
        cell(G_ME0, {R_TFE, (long long)t * TF, (long long)T_in * TF}, {R_FEATS, t * plane, T_in * plane}, t ? Operand{R_H0, (t - 1) * P, plane} : none,
             {R_H0, t * P, plane}, R_C0, "pf::fg::gemm_kernel<9,lstm> enc0", "pf::fg::pair_kernel<lstm> enc0");
    for (int t = 0; t < T_in; ++t)
        cell(G_ME1, {}, {R_H0, t * P, plane}, t ? Operand{R_H1, ((t - 1) & 1) * P, plane} : none, {R_H1, (t & 1) * P, plane}, R_C1,
             "pf::fg::gemm_kernel<9,lstm> enc1", "pf::fg::pair_kernel<lstm> enc1");
    int h0cur = T_in - 1, h1cur = (T_in - 1) & 1;      // the slots that hold each layer's newest h
    auto out_conv = [&](int g, int slot) {             // mask_encoder_out / mask_decoder_out of layer 1's h -> mask_feats[:, slot]
        gemm(g, EPI_BIAS, {R_H1, h1cur * P, plane}, {R_MASK_FEATS, slot * plane, mf_stride}, "pf::fg::gemm_kernel<1,bias> out", nullptr);
    };
    out_conv(G_MEO, 0);                                // current_mask_feats (:282-284)
    // ---- decoder (:289-318)
    for (int t = 0; t < T_out; ++t) {
        const Operand cmf = {R_MASK_FEATS, t * plane, mf_stride}, instd = {R_INSTD, 0, IFH};      // current_mask_feats
        Step &f = add(K_INST_FEAT, "pf::fg::inst_feat_kernel");
        f.x = cmf, f.out = instd, f.t = t;
        Step &d = add(K_TRAJ_DEC, "pf::fg::traj_decoder_kernel");
        d.x = instd, d.out = {R_TFD, 0, TF}, d.c = {R_GRUH, 0, HID}, d.t = t;
        const int h0nxt = (h0cur + 1) % r0, h1nxt = (h1cur + 1) & 1;
        cell(G_MD0, {R_TFD, 0, TF}, cmf, {R_H0, h0cur * P, plane}, {R_H0, h0nxt * P, plane}, R_C0, "pf::fg::gemm_kernel<9,lstm> dec0",
             "pf::fg::pair_kernel<lstm> dec0");
        cell(G_MD1, {}, {R_H0, h0nxt * P, plane}, {R_H1, h1cur * P, plane}, {R_H1, h1nxt * P, plane}, R_C1, "pf::fg::gemm_kernel<9,lstm> dec1",
             "pf::fg::pair_kernel<lstm> dec1");
        h0cur = h0nxt, h1cur = h1nxt;
        out_conv(G_MDO, t + 1);
    }
    // ---- mask head on the selected step (:334-336)
    Step &ga = add(K_GATHER, nullptr);
    ga.x = {R_MASK_FEATS, 0, mf_stride}, ga.out = {R_OUTPUT_FEATS, 0, plane};
    Operand src = ga.out;
    for (int i = 0; i < 4; ++i) {
        const Operand dst = {i & 1 ? R_YB : R_YA, 0, plane};
        gemm(G_F1 + i, EPI_RELU, src, dst, "pf::fg::gemm_kernel<9,relu> mask_fcn", "pf::fg::pair_kernel<relu> mask_fcn");
        src = dst;
    }
    gemm(G_DC, EPI_DECONV, src, {R_YD, 0, C * 784LL}, "pf::fg::gemm_kernel<1,deconv>", nullptr);
    Step &pr = add(K_PREDICT, "pf::fg::predictor_kernel");
    pr.x = {R_YD, 0, C * 784LL}, pr.out = {R_MASKS, 0, 784};
    // pair launches: the GEMM's section of the pair weights, the next three slots; a source boundary inside a channel octet has no pair form
    for (Step &st : steps) {
        if (st.kind != K_PAIR) continue;
        st.pair = (int)(std::find(kPairGemm, kPairGemm + NPAIR, st.gemm) - kPairGemm);
        st.slot = slots++;
        if (st.pair == NPAIR || st.nvec % 8 || st.nx % 8 || st.nh % 8 || FG_SLOT0 + 3 * slots > FG_STATUS_WORDS)
            rc = fail(PF_EINVAL, "pf_fg: %s has no pair form", st.label);
    }
    return rc;
}

}  // namespace fg
}  // namespace pf

using namespace pf;
using namespace pf::fg;

extern "C" int pf_fg_weights_size(int flags, size_t *raw_floats, size_t *packed_floats) {
    if (!raw_floats || !packed_floats) return fail(PF_EINVAL, "pf_fg_weights_size: null output");
    if (int rc = check_dims(0, 1, 1, flags)) return rc;
    const Layout L = layout();
    *raw_floats = L.raw_total;
    *packed_floats = (flags & PF_FG_PAIR) ? pair_layout(L).total : L.total;
    return 0;
}

extern "C" int pf_fg_workspace(int N, int T_in, int T_out, int flags, size_t *bytes) {
    if (!bytes) return fail(PF_EINVAL, "pf_fg_workspace: null output");
    // flags = 0 only, as ever: the workspace of a PF_FG_PAIR forward has a size call of its own
    if (int rc = check_dims(N, T_in, T_out, flags, 0)) return rc;
    *bytes = ws_layout(N, T_in, 0).total;
    return 0;
}

extern "C" int pf_fg_pair_workspace(int N, int T_in, int T_out, size_t *bytes) {
    if (!bytes) return fail(PF_EINVAL, "pf_fg_pair_workspace: null output");
    if (int rc = check_dims(N, T_in, T_out, PF_FG_PAIR)) return rc;
    *bytes = ws_layout(N, T_in, PF_FG_PAIR).total;
    return 0;
}

// floats per instance of a step's operands, from the fields the enqueue loop hands to the kernels: {vec, x, h, out, c}
static void extents(const Step &st, int T_in, int T_out, long long (&e)[5]) {
    const long long plane = (long long)C * HW, T = st.t < 0 ? T_in : 1;
    std::fill(e, e + 5, 0);
    switch (st.kind) {
        case K_GEMM: case K_PAIR:
            e[0] = st.nvec, e[1] = st.nx * (long long)HW, e[2] = st.nh * (long long)HW;
            e[3] = (long long)kGemm[st.gemm].tiles * (st.epi == EPI_LSTM ? 16 : 64) * HW, e[4] = plane;
            break;
        case K_INST_FEAT: e[1] = T * plane, e[3] = T * IFH; break;
        case K_TRAJ_ENC: case K_TRAJ_DEC: e[1] = T * IFH, e[3] = T * TF, e[4] = HID; break;
        case K_GATHER: e[1] = (1 + T_out) * plane, e[3] = plane; break;      // one of slots 1 .. T_out, chosen on the device
        case K_PREDICT: e[1] = C * 784LL, e[3] = 784; break;
        default: break;
    }
}

extern "C" int pf_debug_fg_schedule(int N, int T_in, int T_out, int flags, long long *regions, int cap_regions, int *n_regions,
                                    long long *steps, char *labels, int cap_steps, int *n_steps) {
    if (!n_regions || !n_steps || (cap_regions > 0 && !regions) || (cap_steps > 0 && !steps))
        return fail(PF_EINVAL, "pf_debug_fg_schedule: bad argument");
    std::vector<Step> sched;
    if (int rc = build_fg_schedule(N, T_in, T_out, flags, sched)) return rc;
    const Ws W = ws_layout(N, T_in, flags);
    *n_regions = R_FEATS;
    for (int r = R_STATUS; r <= R_FEATS && r - 1 < cap_regions; ++r) {
        const long long row[3] = {r < R_FEATS ? r : R_NONE, r < R_FEATS ? (long long)(W.off[r] * sizeof(float)) : 0,
                                  r < R_FEATS ? (long long)(W.floats[r] * sizeof(float)) : (long long)W.total};
        std::copy(row, row + 3, regions + 3 * (r - 1));
    }
    *n_steps = (int)sched.size();
    for (size_t i = 0; i < sched.size() && (int)i < cap_steps; ++i) {
        const Step &st = sched[i];
        long long e[5], *row = steps + 30 * i;
        extents(st, T_in, T_out, e);
        const long long head[10] = {st.kind, st.gemm, st.epi, st.nvec, st.nx, st.nh, st.gemm < 0 ? 0 : kGemm[st.gemm].ctot, st.pair, st.slot, st.t};
        std::copy(head, head + 10, row);
        const Operand *ops[5] = {&st.vec, &st.x, &st.h, &st.out, &st.c};
        for (int k = 0; k < 5; ++k) {
            const long long o[4] = {ops[k]->region, ops[k]->off, ops[k]->stride, ops[k]->region ? e[k] : 0};
            std::copy(o, o + 4, row + 10 + 4 * k);
        }
        if (labels) strncpy(labels + 64 * i, st.label ? st.label : "", 64);
    }
    return PF_OK;
}
