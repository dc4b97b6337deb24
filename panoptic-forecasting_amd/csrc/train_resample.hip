// Copies and resampling transposes of the training step: the padded copies around an odd-width convolution, zero-stuffing and
// channel zeroing for backward-data, average-pool and bilinear-upsample backward.
#include "conv_epilogue.h"
#include "pf_prof.h"
#include "train_device.h"
#include "train_kernels.h"

namespace pf {

// ---- widths that are not a multiple of 4 (the 50- and 25-pixel levels of an 800 x 800 crop): the LDS-DMA kernels move
// 16-B pieces and need 16-B aligned rows.  Such a conv runs on COPIES with the row pitch rounded up to 4: its input ranges
// gathered into one contiguous tensor [B][Cin][H][Wp] with zero pad columns (= the convolution's own zero padding, so the
// real columns of the result are unchanged), its result [B][Cout][Hout][Wop] scattered back into the destination slice
// (accumulating for backward-data).  Two small copy kernels around a fast conv instead of the register-staged generic
// kernel (1.7-16 TFLOP/s on these levels: 14 ms of a 44 ms step).
struct PadGatherArgs {
    const float *src[kConvMaxSrc];
    int ctotal[kConvMaxSrc], choff[kConvMaxSrc], cstart[kConvMaxSrc + 1], n_src;
};
__global__ __launch_bounds__(256) void pad_gather_kernel(PadGatherArgs g, int Cin, int H, int W, int Wp, float *dst) {
    const int bc = blockIdx.y, b = bc / Cin, c = bc - b * Cin;
    const int i4 = blockIdx.x * 256 + threadIdx.x;          // 4-column group of the padded plane
    const int wp4 = Wp / 4;
    if (i4 >= H * wp4) return;
    const int y = i4 / wp4, x = (i4 - y * wp4) * 4;
    int j = 0;
    while (j + 1 < g.n_src && c >= g.cstart[j + 1]) ++j;
    const float *sp = g.src[j] + ((long long)b * g.ctotal[j] + g.choff[j] + (c - g.cstart[j])) * H * W + (long long)y * W;
    tr_f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = x + k < W ? sp[x + k] : 0.f;
    *reinterpret_cast<tr_f32x4 *>(dst + ((long long)bc * H + y) * Wp + x) = v;
}
__global__ __launch_bounds__(256) void unpad_scatter_kernel(const float *src, int C, int H, int W, int Wp, float *dst, int dst_ctotal, int dst_choff,
                                                            int accum) {
    const int bc = blockIdx.y, b = bc / C, c = bc - b * C;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    float *d = dst + ((long long)b * dst_ctotal + dst_choff + c) * H * W + i;
    const float v = src[((long long)bc * H + y) * Wp + x];
    *d = accum ? *d + v : v;
}
// the result of ONE backward-data convolution over all input ranges of a layer ([B][C][H][Wp]) added to the gradient of each
// range's tensor (a null destination - the network input - is skipped)
struct ScatterArgs {
    float *dst[kConvMaxSrc];
    int ctotal[kConvMaxSrc], choff[kConvMaxSrc], cstart[kConvMaxSrc + 1], overwrite[kConvMaxSrc], n;
};
__global__ __launch_bounds__(256) void unpad_scatter_multi_kernel(const float *src, int C, int H, int W, int Wp, ScatterArgs t) {
    const int bc = blockIdx.y, b = bc / C, c = bc - b * C;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * W) return;
    int j = 0;
    while (j + 1 < t.n && c >= t.cstart[j + 1]) ++j;
    if (!t.dst[j]) return;
    const int y = i / W, x = i - y * W;
    float *d = t.dst[j] + ((long long)b * t.ctotal[j] + t.choff[j] + (c - t.cstart[j])) * H * W + i;
    const float v = src[((long long)bc * H + y) * Wp + x];
    *d = t.overwrite[j] ? v : *d + v;
}
int launch_unpad_scatter_multi(const float *src, int B, int C, int H, int W, int Wp, float *const *dst, const int *ctotal, const int *choff,
                               const int *ch, const int *overwrite, int n, hipStream_t s) {
    if (n < 1 || n > kConvMaxSrc) return fail(PF_EINVAL, "unpad_scatter_multi: %d ranges", n);
    ScatterArgs t = {};
    t.n = n;
    int c0 = 0;
    for (int j = 0; j < n; ++j) {
        t.dst[j] = dst[j]; t.ctotal[j] = ctotal[j]; t.choff[j] = choff[j]; t.cstart[j] = c0; t.overwrite[j] = overwrite[j];
        c0 += ch[j];
    }
    for (int j = n; j <= kConvMaxSrc; ++j) t.cstart[j] = c0;
    if (c0 != C) return fail(PF_EINVAL, "unpad_scatter_multi: ranges cover %d of %d channels", c0, C);
    hipLaunchKernelGGL(unpad_scatter_multi_kernel, dim3((unsigned)((H * W + 255) / 256), B * C), dim3(256), 0, s, src, C, H, W, Wp, t);
    PF_LAUNCH_CHECK("unpad_scatter_multi_kernel");
    return PF_OK;
}
// zeros in channels [c0, c0 + n) of a [B][ctotal][HW] tensor (the few gradient channels whose first writer accumulates)
__global__ __launch_bounds__(256) void zero_channels_kernel(float *t, long long run, long long batch_stride) {
    float *p = t + (long long)blockIdx.y * batch_stride;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < run; i += (long long)gridDim.x * 256) p[i] = 0.f;
}
int launch_zero_channels(float *t, int B, int ctotal, int c0, int n, long long HW, hipStream_t s) {
    const long long run = (long long)n * HW;
    long long blocks = (run + 1023) / 1024;
    blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
    hipLaunchKernelGGL(zero_channels_kernel, dim3((unsigned)blocks, B), dim3(256), 0, s, t + (long long)c0 * HW, run, (long long)ctotal * HW);
    PF_LAUNCH_CHECK("zero_channels_kernel");
    return PF_OK;
}
int launch_pad_gather(const ConvArgs &a, int B, int Wp, float *dst, hipStream_t s) {
    PadGatherArgs g;
    g.n_src = a.n_src;
    for (int j = 0; j < kConvMaxSrc; ++j) {
        g.src[j] = a.src[j]; g.ctotal[j] = a.src_ctotal[j]; g.choff[j] = a.src_choff[j]; g.cstart[j] = a.src_cstart[j];
    }
    g.cstart[kConvMaxSrc] = a.src_cstart[kConvMaxSrc];
    hipLaunchKernelGGL(pad_gather_kernel, dim3((unsigned)((a.Hin * (Wp / 4) + 255) / 256), B * a.Cin), dim3(256), 0, s, g, a.Cin, a.Hin, a.Win, Wp, dst);
    PF_LAUNCH_CHECK("pad_gather_kernel");
    return PF_OK;
}
int launch_unpad_scatter(const float *src, int B, int C, int H, int W, int Wp, float *dst, int dst_ctotal, int dst_choff, int accum, hipStream_t s) {
    hipLaunchKernelGGL(unpad_scatter_kernel, dim3((unsigned)((H * W + 255) / 256), B * C), dim3(256), 0, s, src, C, H, W, Wp, dst, dst_ctotal, dst_choff,
                       accum);
    PF_LAUNCH_CHECK("unpad_scatter_kernel");
    return PF_OK;
}

// zero-stuffing for the backward-data pass of a stride-2 conv: up[b][c][2*oy][2*ox] = dy[b][c][oy][ox], zeros elsewhere
__global__ __launch_bounds__(256) void zero_stuff_kernel(const float *dy, int Hout, int Wout, int Hin, int Win, float *up) {
    const int bc = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)Hin * Win) return;
    const int y = (int)(i / Win), x = (int)(i - (long long)y * Win);
    float v = 0.f;
    if (!(y & 1) && !(x & 1) && (y >> 1) < Hout && (x >> 1) < Wout) v = dy[((long long)bc * Hout + (y >> 1)) * Wout + (x >> 1)];
    up[(long long)bc * Hin * Win + i] = v;
}
int launch_zero_stuff(const float *dy, int planes, int Hout, int Wout, int Hin, int Win, float *up, hipStream_t s) {
    ProfScope ps(s, "zero_stuff_kernel", 0.0, 4.0 * planes * ((double)Hout * Wout + (double)Hin * Win));
    hipLaunchKernelGGL(zero_stuff_kernel, dim3((unsigned)(((long long)Hin * Win + 255) / 256), planes), dim3(256), 0, s, dy, Hout, Wout, Hin, Win, up);
    PF_LAUNCH_CHECK("zero_stuff_kernel");
    return PF_OK;
}

// ------------------------------------------------------------------------------------------------ pool / upsample backward
// AvgPool2d(2,2): gin[2y+dy][2x+dx] += 0.25 * gout[y][x]   (rows/cols dropped by the floor division get no gradient)
__global__ __launch_bounds__(256) void avgpool2_bwd_kernel(const float *gout, int Hin, int Win, int overwrite, float *gin) {
    const int bc = blockIdx.y, Ho = Hin >> 1, Wo = Win >> 1;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)Hin * Win) return;
    const int y = (int)(i / Win), x = (int)(i - (long long)y * Win);
    const float v = ((y >> 1) < Ho && (x >> 1) < Wo) ? 0.25f * gout[((long long)bc * Ho + (y >> 1)) * Wo + (x >> 1)] : 0.f;
    float *d = gin + (long long)bc * Hin * Win + i;
    if (overwrite) *d = v;
    else *d += v;
}
int launch_avgpool2_bwd(const float *gout, int planes, int Hin, int Win, int overwrite, float *gin, hipStream_t s) {
    hipLaunchKernelGGL(avgpool2_bwd_kernel, dim3((unsigned)(((long long)Hin * Win + 255) / 256), planes), dim3(256), 0, s, gout, Hin, Win, overwrite, gin);
    PF_LAUNCH_CHECK("avgpool2_bwd_kernel");
    return PF_OK;
}

// transpose of bilinear align_corners=True interpolation, gather form (deterministic): every source pixel sums the output
// pixels whose two taps per axis (lin_coord, the same function the forward kernels use) include it.
// Candidate outputs of source index i along one axis (scale = source step per output, n_out outputs): r = scale * o in
// (i - 1, i + 1)  ->  widened by one on both sides; upsample_tap_weight tests the indices exactly
__device__ __forceinline__ void upsample_bwd_range(int i, float scale, int n_out, int &lo, int &hi) {
    lo = 0, hi = n_out - 1;
    if (scale > 0.f) {
        lo = max(0, (int)floorf((float)(i - 1) / scale) - 1);
        hi = min(n_out - 1, (int)ceilf((float)(i + 1) / scale) + 1);
    }
}
// weight of output index o on source index i
__device__ __forceinline__ float upsample_tap_weight(int o, float scale, int n_in, int i) {
    int i0, i1;
    float w0, w1;
    lin_coord(o, scale, n_in, i0, i1, w0, w1);
    return (i0 == i ? w0 : 0.f) + (i1 == i ? w1 : 0.f);
}
__global__ __launch_bounds__(256) void upsample_bwd_kernel(const float *gout, int Hi, int Wi, int Ho, int Wo, float sh, float sw,
                                                           const double *inv_count /* nullable: multiply by scale / *inv_count */, float scale,
                                                           int accumulate, float *gin) {
    const int bc = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)Hi * Wi) return;
    const int iy = (int)(i / Wi), ix = (int)(i - (long long)iy * Wi);
    int oy_lo, oy_hi, ox_lo, ox_hi;
    upsample_bwd_range(iy, sh, Ho, oy_lo, oy_hi);
    upsample_bwd_range(ix, sw, Wo, ox_lo, ox_hi);
    const float *gp = gout + (long long)bc * Ho * Wo;
    float sum = 0.f;
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
        const float wy = upsample_tap_weight(oy, sh, Hi, iy);
        if (wy == 0.f) continue;
        float rs = 0.f;
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
            const float wx = upsample_tap_weight(ox, sw, Wi, ix);
            if (wx != 0.f) rs += wx * gp[(long long)oy * Wo + ox];
        }
        sum += wy * rs;
    }
    if (inv_count) sum = (float)((double)sum * (double)scale / fmax(*inv_count, 1.0));
    float *d = gin + (long long)bc * Hi * Wi + i;
    *d = accumulate ? *d + sum : sum;
}
// The same sum as two passes over a [planes][Ho][Wi] scratch - rows first (tmp[oy][ix] = sum_ox wx g[oy][ox]), then columns
// (gin[iy][ix] = sum_oy wy tmp[oy][ix]): the nesting and the order of the one-pass kernel's own loops over the same two helpers,
// so the same bits, with ~10 + 10 taps per source pixel instead of ~10 x 10 (the 4x head of the loss: 0.45 -> 0.1x ms)
__global__ __launch_bounds__(256) void upsample_bwd_rows_kernel(const float *gout, int Wi, int Ho, int Wo, float sw, float *tmp) {
    const int bc = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)Ho * Wi) return;
    const int oy = (int)(i / Wi), ix = (int)(i - (long long)oy * Wi);
    int ox_lo, ox_hi;
    upsample_bwd_range(ix, sw, Wo, ox_lo, ox_hi);
    const float *row = gout + ((long long)bc * Ho + oy) * Wo;
    float rs = 0.f;
    for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        const float wx = upsample_tap_weight(ox, sw, Wi, ix);
        if (wx != 0.f) rs += wx * row[ox];
    }
    tmp[(long long)bc * Ho * Wi + i] = rs;
}
__global__ __launch_bounds__(256) void upsample_bwd_cols_kernel(const float *tmp, int Hi, int Wi, int Ho, float sh, const double *inv_count,
                                                                float scale, int accumulate, float *gin) {
    const int bc = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)Hi * Wi) return;
    const int iy = (int)(i / Wi), ix = (int)(i - (long long)iy * Wi);
    int oy_lo, oy_hi;
    upsample_bwd_range(iy, sh, Ho, oy_lo, oy_hi);
    const float *tp = tmp + (long long)bc * Ho * Wi + ix;
    float sum = 0.f;
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
        const float wy = upsample_tap_weight(oy, sh, Hi, iy);
        if (wy == 0.f) continue;
        sum += wy * tp[(long long)oy * Wi];
    }
    if (inv_count) sum = (float)((double)sum * (double)scale / fmax(*inv_count, 1.0));
    float *d = gin + (long long)bc * Hi * Wi + i;
    *d = accumulate ? *d + sum : sum;
}
size_t upsample_bwd_tmp_floats(int planes, int Hi, int Wi, int Ho, int Wo) {
    return (long long)planes * Ho * Wo >= (1ll << 22) ? (size_t)planes * Ho * Wi : 0;     // small planes: one pass, one launch
}
int launch_upsample_bwd(const float *gout, int planes, int Hi, int Wi, int Ho, int Wo, const double *count, float scale, int accumulate,
                        float *gin, float *tmp, hipStream_t s) {
    const float sh = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f, sw = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f;
    if (tmp && upsample_bwd_tmp_floats(planes, Hi, Wi, Ho, Wo)) {
        hipLaunchKernelGGL(upsample_bwd_rows_kernel, dim3((unsigned)(((long long)Ho * Wi + 255) / 256), planes), dim3(256), 0, s, gout, Wi, Ho, Wo, sw, tmp);
        hipLaunchKernelGGL(upsample_bwd_cols_kernel, dim3((unsigned)(((long long)Hi * Wi + 255) / 256), planes), dim3(256), 0, s, tmp, Hi, Wi, Ho, sh,
                           count, scale, accumulate, gin);
        PF_LAUNCH_CHECK("upsample_bwd_rows/cols_kernel");
        return PF_OK;
    }
    hipLaunchKernelGGL(upsample_bwd_kernel, dim3((unsigned)(((long long)Hi * Wi + 255) / 256), planes), dim3(256), 0, s, gout, Hi, Wi, Ho, Wo, sh, sw,
                       count, scale, accumulate, gin);
    PF_LAUNCH_CHECK("upsample_bwd_kernel");
    return PF_OK;
}

}  // namespace pf
