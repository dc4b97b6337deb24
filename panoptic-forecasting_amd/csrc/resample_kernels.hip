// Pool and upsample of the bg network as launches of their own (HBM-bound, VALU only); the training plan calls them too:
//   avgpool2_kernel : nn.AvgPool2d(2,2)                     hardnet.py:296
//   upsample_kernel : F.interpolate(bilinear, align_corners) hardnet.py:248-253
#include "net_kernels.h"
#include "conv_epilogue.h"
#include "pf_prof.h"

namespace pf {

__global__ __launch_bounds__(256) void avgpool2_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                       int planes, int Hin, int Win, int Hout, int Wout, unsigned *status, unsigned *slot) {
    float vmax = 0.f;
    const size_t total = (size_t)planes * Hout * Wout;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int x = (int)(i % Wout);
        const size_t r = i / Wout;
        const int y = (int)(r % Hout);
        const size_t p = r / Hout;
        const float *s = src + (p * Hin + 2 * y) * (size_t)Win + 2 * x;
        const float v = (((s[0] + s[1]) + s[Win]) + s[Win + 1]) * 0.25f;
        dst[i] = v;
        vmax = fmaxf(vmax, fabsf(v));
    }
    range_commit(status, slot, vmax);
}

__global__ __launch_bounds__(256) void upsample_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                       int planes, int Hin, int Win, int Hout, int Wout, unsigned *status, unsigned *slot) {
    float vmax = 0.f;
    const float sh = Hout > 1 ? (float)(Hin - 1) / (float)(Hout - 1) : 0.f;
    const float sw = Wout > 1 ? (float)(Win - 1) / (float)(Wout - 1) : 0.f;
    const size_t total = (size_t)planes * Hout * Wout;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int x = (int)(i % Wout);
        const size_t r = i / Wout;
        const int y = (int)(r % Hout);
        const size_t p = r / Hout;
        int y0, y1, x0, x1;
        float hy0, hy1, lx0, lx1;
        lin_coord(y, sh, Hin, y0, y1, hy0, hy1);
        lin_coord(x, sw, Win, x0, x1, lx0, lx1);
        const float *s = src + p * (size_t)Hin * Win;
        const float t0 = lx0 * s[(size_t)y0 * Win + x0] + lx1 * s[(size_t)y0 * Win + x1];
        const float t1 = lx0 * s[(size_t)y1 * Win + x0] + lx1 * s[(size_t)y1 * Win + x1];
        const float v = hy0 * t0 + hy1 * t1;
        dst[i] = v;
        vmax = fmaxf(vmax, fabsf(v));
    }
    range_commit(status, slot, vmax);
}

int launch_avgpool2(const float *src, float *dst, int planes, int Hin, int Win, unsigned *status, unsigned *slot, hipStream_t s) {
    const int Ho = Hin / 2, Wo = Win / 2;
    ProfScope ps(s, "pf::avgpool2_kernel", 0, 4.0 * planes * ((double)Hin * Win + (double)Ho * Wo));
    hipLaunchKernelGGL(avgpool2_kernel, dim3(grid_for((size_t)planes * Ho * Wo)), dim3(256), 0, s, src, dst, planes,
                       Hin, Win, Ho, Wo, status, slot);
    PF_LAUNCH_CHECK("avgpool2_kernel");
    return PF_OK;
}

int launch_upsample(const float *src, float *dst, int planes, int Hin, int Win, int Hout, int Wout, unsigned *status, unsigned *slot,
                    hipStream_t s) {
    ProfScope ps(s, "pf::upsample_kernel", 0, 4.0 * planes * ((double)Hin * Win + (double)Hout * Wout));
    hipLaunchKernelGGL(upsample_kernel, dim3(grid_for((size_t)planes * Hout * Wout)), dim3(256), 0, s, src, dst,
                       planes, Hin, Win, Hout, Wout, status, slot);
    PF_LAUNCH_CHECK("upsample_kernel");
    return PF_OK;
}

}  // namespace pf
