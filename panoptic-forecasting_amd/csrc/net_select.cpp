// Which kernel a stem, head or validation-loss launch runs, with its grid, LDS size and profile label: host code only.  The launchers
// (stem_kernels.hip, head_kernels.hip) enqueue what these functions return, the schedule asks stem_family whether the stem can feed the
// fused front end, and pf_debug_net_choice (below) hands the same answers to tests without a device.
// The profile label of a launch is the instantiation's name as rocprofv3 prints it, made from the rows of net_kernels.h.
#include <cmath>
#include <cstring>

#include "net_kernels.h"

namespace pf {

namespace {
const char *stem_label(int family, int variant) {
    switch (family * 8 + variant) {
#define X(V, HD, HL, FD) case STEM_V4 * 8 + V: return "void pf::stem_onehot_v4_kernel<3, " #HD ", " #HL ", " #FD ">(pf::StemArgs, float)";
        PF_STEM_V4_INSTANCES(X)
#undef X
#define X(V, S64, HD, HL) case STEM_V3 * 8 + V: return "void pf::stem_onehot_v3_kernel<3, " #S64 ", " #HD ", " #HL ">(pf::StemArgs)";
        PF_STEM_V3_INSTANCES(X)
#undef X
    }
    return "pf::stem_onehot_kernel(pf::StemArgs)";
}
// head_col_kernel<C> / seg_loss_tile_kernel<C>; nullptr: C is not built
const char *tiled_label(bool loss, int C) {
    switch (C) {
#define X(CC) case CC: return loss ? "void pf::seg_loss_tile_kernel<" #CC ">(pf::LossArgs)" : "void pf::head_col_kernel<" #CC ">(pf::HeadArgs)";
        PF_HEAD_CLASSES(X)
#undef X
    }
    return nullptr;
}
// bilinear source step per output pixel, align_corners (the kernels compute the same fp32 value)
float lin_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }
// Bound of the source window a TH x TW output tile stages in LDS, in floats per channel: the tile's first and last pixel lie
// (int)(scale * (T - 1)) source pixels apart at most, + 1 for the far neighbour, + 1 for the count, + 1 for the truncation of the first
size_t window_floats(float sh, int TH, float sw, int TW) { return (size_t)((int)(sh * (TH - 1)) + 3) * (size_t)((int)(sw * (TW - 1)) + 3); }
}  // namespace

// Tries all 65 281 values: the hop quantises depth to a u16 code c in 0..65280 (round(clamp(d + 1, 0, 255) * 256)), so
// x = clamp(c / 256 - 1) - mean takes no others (fmaf of the host libm is exact).
bool stem_fast_div_exact(float mean, float stdv, float dmin, float dmax) {
    static float key[4] = {0.f, 0.f, 0.f, 0.f};
    static int cached = -1;
    if (cached >= 0 && key[0] == mean && key[1] == stdv && key[2] == dmin && key[3] == dmax) return cached != 0;
    bool ok = std::isfinite(stdv) && stdv != 0.f;
    const volatile float r = 1.0f / stdv;
    for (int c = 0; ok && c <= 65280; ++c) {
        float d = (float)c / 256.f - 1.f;
        d = d > 0.f ? fminf(fmaxf(d, dmin), dmax) : -1.f;
        const volatile float x = d - mean;
        const volatile float q0 = x * r;
        const volatile float e = fmaf(-q0, stdv, x);
        const volatile float q1 = fmaf(e, r, q0);
        const volatile float want = x / stdv;
        const float got = q1, w = want;
        ok = memcmp(&got, &w, 4) == 0;
    }
    key[0] = mean; key[1] = stdv; key[2] = dmin; key[3] = dmax;
    cached = ok ? 1 : 0;
    return ok;
}

// T = 3 with the plan's re-packed weights and 32-bit lane offsets: v3, or v4 (2 x 2 outputs per lane, the only kernel that writes the
// packed-pair layout) for u8 labels on an image of whole 4 x 4 blocks; everything else (T != 3, T*H*W >= 2^32) runs the generic
// kernel, which indexes with size_t
int stem_family(const StemArgs &a) {
    const bool v3 = a.T == 3 && a.wdep && a.woh && (unsigned long long)a.T * a.H * a.W < (1ull << 32);
    const bool v4 = v3 && !a.seg_is_i64 && (a.W & 3) == 0 && (a.H & 3) == 0 && a.Wout * 2 == a.W && a.Hout * 2 == a.H;
    return v4 ? STEM_V4 : v3 ? STEM_V3 : STEM_GENERIC;
}

int choose_stem(const StemArgs &a, StemChoice *c) {
    const size_t lds = (size_t)9 * a.T * (a.n_cls + 1) * kStemRow * sizeof(float);
    if (lds > 60000) return fail(PF_EUNSUPPORTED, "stem: T=%d n_cls=%d weights exceed LDS budget", a.T, a.n_cls);
    c->family = stem_family(a);
    const bool v4 = c->family == STEM_V4, v3 = c->family == STEM_V3;
    if (a.dst_fmt && !v4) return fail(PF_EUNSUPPORTED, "stem: these arguments select a kernel that writes fp32 only");
    c->seg64 = a.seg_is_i64 != 0;
    c->hop_d = (a.hop & PF_HOP_DEPTH_U16) != 0;
    c->hop_lut = (a.hop & PF_HOP_TRAINID_LUT) != 0;
    // the reciprocal form of the division is exact only on the value set of the hop (proven per parameter set)
    c->fast_div = v4 && c->hop_d && stem_fast_div_exact(a.depth_mean, a.depth_std, a.min_depth, a.max_depth);
    c->variant = v4 ? c->hop_d * 4 + c->hop_lut * 2 + c->fast_div : v3 ? c->seg64 * 4 + c->hop_d * 2 + c->hop_lut : 0;
    c->grid = v4 ? dim3((a.Wout + 127) / 128, (a.Hout + 7) / 8, a.B) : dim3((a.Wout + 63) / 64, (a.Hout + 3) / 4, a.B);
    c->lds = lds;
    c->label = stem_label(c->family, c->variant);
    return PF_OK;
}

HeadChoice choose_head(const HeadArgs &a) {
    const float sh = lin_scale(a.Hin, a.Hout), sw = lin_scale(a.Win, a.Wout);
    const size_t lds = window_floats(sh, kHeadCH, sw, kHeadCW) * sizeof(float) * a.C;
    const char *col = tiled_label(false, a.C);
    if (col && a.Hin >= 2 && a.Win >= 2 && lds <= kHeadLdsMax)
        return {HEAD_TILED, dim3((a.Wout + kHeadCW - 1) / kHeadCW, (a.Hout + kHeadCH - 1) / kHeadCH, a.B), lds, col};
    // 4 consecutive outputs span <= 2 source columns
    if ((a.Wout & 3) == 0 && 3.f * sw < 1.f && a.Win >= 3)
        return {HEAD_QUAD, dim3(grid_for((size_t)a.B * a.Hout * (a.Wout >> 2))), 0, "pf::head4_kernel(pf::HeadArgs)"};
    return {HEAD_PLAIN, dim3(grid_for((size_t)a.B * a.Hout * a.Wout)), 0, "pf::head_kernel(pf::HeadArgs)"};
}

void seg_loss_geometry(int B, int Hout, int Wout, LossChoice *c) {
    c->grid = dim3((Wout + kHeadTW - 1) / kHeadTW, (Hout + kHeadTH - 1) / kHeadTH, B);
    c->blocks = (size_t)c->grid.x * c->grid.y * c->grid.z;
    c->ws_bytes = align_up(c->blocks * 3 * sizeof(double), 256);
}

int choose_seg_loss(int B, int C, int Hin, int Win, int Hout, int Wout, LossChoice *c) {
    if (!(c->label = tiled_label(true, C))) return fail(PF_EUNSUPPORTED, "pf_seg_loss: built for 11 or 19 classes, got %d", C);
    seg_loss_geometry(B, Hout, Wout, c);
    c->lds = window_floats(lin_scale(Hin, Hout), kHeadTH, lin_scale(Win, Wout), kHeadTW) * C * sizeof(float);
    if (c->lds > kHeadLdsMax)
        return fail(PF_EUNSUPPORTED, "pf_seg_loss: source window of %zu B per tile does not fit LDS (downsampling heads are not built)", c->lds);
    return PF_OK;
}

}  // namespace pf

extern "C" int pf_debug_net_choice(int what, const int *iargs, int n_iargs, const float *fargs, int n_fargs, char *label, size_t label_cap,
                                   long long *out, int cap) {
    if (!iargs || !out || cap < 8 || (label_cap && !label)) return pf::fail(PF_EINVAL, "pf_debug_net_choice: bad arguments (8 numbers of output)");
    long long v[8] = {0, 0, 0, 0, pf::kNetBlock, 0, 0, 0};
    const char *name = nullptr;
    dim3 grid;
    if (what == 0 && n_iargs == 11 && fargs && n_fargs == 4) {
        static const float packed[4] = {0.f, 0.f, 0.f, 0.f};   // an address for the plan's re-packed weights; nothing is read through it
        pf::StemArgs a{};
        a.T = iargs[0]; a.n_cls = iargs[1]; a.H = iargs[2]; a.W = iargs[3]; a.Hout = iargs[4]; a.Wout = iargs[5]; a.B = iargs[6];
        a.seg_is_i64 = iargs[7]; a.hop = iargs[8]; a.dst_fmt = iargs[9];
        a.wdep = a.woh = iargs[10] ? packed : nullptr;
        a.depth_mean = fargs[0]; a.depth_std = fargs[1]; a.min_depth = fargs[2]; a.max_depth = fargs[3];
        pf::StemChoice c;
        if (int rc = pf::choose_stem(a, &c)) return rc;
        v[0] = c.family; v[5] = (long long)c.lds; v[6] = c.seg64 * 1 + c.hop_d * 2 + c.hop_lut * 4 + c.fast_div * 8; v[7] = c.variant;
        grid = c.grid; name = c.label;
    } else if (what == 1 && n_iargs == 6) {
        pf::HeadArgs a{};
        a.B = iargs[0]; a.C = iargs[1]; a.Hin = iargs[2]; a.Win = iargs[3]; a.Hout = iargs[4]; a.Wout = iargs[5];
        const pf::HeadChoice c = pf::choose_head(a);
        v[0] = c.kind; v[5] = (long long)c.lds; v[6] = a.C;
        grid = c.grid; name = c.label;
    } else if (what == 2 && n_iargs == 6) {
        pf::LossChoice c{};
        if (int rc = pf::choose_seg_loss(iargs[0], iargs[1], iargs[2], iargs[3], iargs[4], iargs[5], &c)) return rc;
        v[5] = (long long)c.lds; v[6] = (long long)c.blocks; v[7] = (long long)c.ws_bytes;
        grid = c.grid; name = c.label;
    } else {
        return pf::fail(PF_EINVAL, "pf_debug_net_choice: what = %d with %d ints and %d floats", what, n_iargs, n_fargs);
    }
    v[1] = grid.x; v[2] = grid.y; v[3] = grid.z;
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    if (label_cap) {
        strncpy(label, name, label_cap - 1);
        label[label_cap - 1] = 0;
    }
    return PF_OK;
}
