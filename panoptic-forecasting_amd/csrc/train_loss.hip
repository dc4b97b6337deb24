// The two ends of the backward chain: bilinear-upsampled cross entropy with its gradient, and global-norm / value clipping
// with SGD (momentum, weight decay).
#include "conv_epilogue.h"
#include "pf_prof.h"
#include "train_device.h"
#include "train_kernels.h"

namespace pf {

// ------------------------------------------------------------------------------------------------ loss
// F.interpolate(logits, (Ho,Wo), bilinear, align_corners=True) -> CrossEntropyLoss(ignore_index) (bg_model.py:44,81) and
// its gradient w.r.t. the upsampled logits, (softmax - onehot) on valid pixels (NOT yet divided by the valid count),
// plus the accuracy counters of :82-84.  partial[block][3] = {sum nll, valid, correct} in fp64.
template <int C>
__global__ __launch_bounds__(256) void ce_fwd_bwd_kernel(const float *logits, int Hi, int Wi, const void *labels, int lab_i64, int Ho, int Wo,
                                                         int ignore, float sh, float sw, float *dfull, double *partial) {
    const int b = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long HWo = (long long)Ho * Wo;
    double v[3] = {0.0, 0.0, 0.0};
    if (i < HWo) {
        const int oy = (int)(i / Wo), ox = (int)(i - (long long)oy * Wo);
        int y0, y1, x0, x1;
        float hy0, hy1, lx0, lx1;
        lin_coord(oy, sh, Hi, y0, y1, hy0, hy1);
        lin_coord(ox, sw, Wi, x0, x1, lx0, lx1);
        const long long li = (long long)b * HWo + i;
        const long long lab = lab_i64 ? reinterpret_cast<const long long *>(labels)[li] : (long long)reinterpret_cast<const uint8_t *>(labels)[li];
        float z[C];
        float mx = -INFINITY;
        int arg = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float *p = logits + ((long long)b * C + c) * Hi * Wi;
            const float t0 = lx0 * p[(long long)y0 * Wi + x0] + lx1 * p[(long long)y0 * Wi + x1];
            const float t1 = lx0 * p[(long long)y1 * Wi + x0] + lx1 * p[(long long)y1 * Wi + x1];
            z[c] = hy0 * t0 + hy1 * t1;
            if (z[c] > mx) { mx = z[c]; arg = c; }
        }
        const bool valid = lab != ignore && lab >= 0 && lab < C;
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) se += expf(z[c] - mx);
        const float lse = mx + logf(se);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float p = expf(z[c] - lse);
            dfull[((long long)b * C + c) * HWo + i] = valid ? (p - (c == lab ? 1.f : 0.f)) : 0.f;
            if (valid && c == lab) v[0] = (double)(lse - z[c]);
        }
        if (lab != ignore) {          // :83-84: total counts labels != 255, correct compares the argmax with the label
            v[1] = 1.0;
            v[2] = arg == lab ? 1.0 : 0.0;
        }
    }
    block_reduce_d<3>(v);
    if (threadIdx.x == 0) {
        double *p = partial + ((long long)b * gridDim.x + blockIdx.x) * 3;
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
    }
}
__global__ __launch_bounds__(256) void sum3_kernel(const double *partial, long long n, double *out3) {
    double v[3] = {0.0, 0.0, 0.0};
    for (long long i = threadIdx.x; i < n; i += 256) {
        v[0] += partial[i * 3 + 0]; v[1] += partial[i * 3 + 1]; v[2] += partial[i * 3 + 2];
    }
    block_reduce_d<3>(v);
    if (threadIdx.x == 0) { out3[0] = v[0]; out3[1] = v[1]; out3[2] = v[2]; }
}
size_t ce_partial_doubles(int B, int Ho, int Wo) { return (size_t)B * (((size_t)Ho * Wo + 255) / 256) * 3; }

int launch_ce_fwd_bwd(const float *logits, int B, int C, int Hi, int Wi, const void *labels, int lab_i64, int Ho, int Wo, int ignore,
                      float *dfull, double *partial, double *out3, hipStream_t s) {
    const float sh = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f, sw = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f;
    const dim3 grid((unsigned)(((long long)Ho * Wo + 255) / 256), B);
    char label[32];
    snprintf(label, sizeof(label), "ce_fwd_bwd_kernel<%d>", C);
    ProfScope ps(s, label, 0.0, 4.0 * B * C * ((double)Hi * Wi + (double)Ho * Wo));
    if (C == 11) hipLaunchKernelGGL((ce_fwd_bwd_kernel<11>), grid, dim3(256), 0, s, logits, Hi, Wi, labels, lab_i64, Ho, Wo, ignore, sh, sw, dfull, partial);
    else if (C == 19) hipLaunchKernelGGL((ce_fwd_bwd_kernel<19>), grid, dim3(256), 0, s, logits, Hi, Wi, labels, lab_i64, Ho, Wo, ignore, sh, sw, dfull, partial);
    else return fail(PF_EUNSUPPORTED, "cross entropy kernels are built for 11 or 19 classes, got %d", C);
    hipLaunchKernelGGL(sum3_kernel, dim3(1), dim3(256), 0, s, partial, (long long)grid.x * B, out3);
    PF_LAUNCH_CHECK("ce_fwd_bwd");
    return PF_OK;
}

// ------------------------------------------------------------------------------------------------ optimiser
// nn.utils.clip_grad_norm_ (train.py:207-208): coef = min(1, max_norm / (||g||_2 + 1e-6)) over the trainable elements
constexpr int kNormBlocks = 512;
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float *g, const uint8_t *trainable, long long n, double *partial) {
    double v[1] = {0.0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)kNormBlocks * 256)
        if (trainable[i]) v[0] += (double)g[i] * (double)g[i];
    block_reduce_d<1>(v);
    if (threadIdx.x == 0) partial[blockIdx.x] = v[0];
}
__global__ __launch_bounds__(256) void clip_coef_kernel(const double *partial, float max_norm, float *coef_norm2 /* [2]: coef, total norm */) {
    double v[1] = {0.0};
    for (int i = threadIdx.x; i < kNormBlocks; i += 256) v[0] += partial[i];
    block_reduce_d<1>(v);
    if (threadIdx.x == 0) {
        const double norm = sqrt(v[0]);
        const double c = (double)max_norm / (norm + 1e-6);
        coef_norm2[0] = max_norm > 0.f ? (float)(c < 1.0 ? c : 1.0) : 1.f;
        coef_norm2[1] = (float)norm;
    }
}
// torch.optim.SGD (train.py:138): g += wd * p;  buf = first ? g : momentum * buf + g;  p -= lr * buf
__global__ __launch_bounds__(256) void sgd_kernel(float *theta, float *grad, float *mom, const uint8_t *trainable, long long n, float lr,
                                                  float momentum, float wd, const float *coef, float clip_value, int first) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !trainable[i]) return;
    float g = grad[i] * coef[0];
    if (clip_value > 0.f) g = fminf(fmaxf(g, -clip_value), clip_value);     // clip_grad_value_ (train.py:205-206)
    grad[i] = g;                                                            // what .grad holds after clipping
    g += wd * theta[i];
    const float buf = (first || momentum == 0.f) ? g : momentum * mom[i] + g;
    mom[i] = buf;
    theta[i] -= lr * buf;
}
size_t sgd_ws_bytes() { return kNormBlocks * sizeof(double) + 64; }

int launch_sgd(float *theta, float *grad, float *mom, const uint8_t *trainable, long long n, float lr, float momentum, float wd, float clip_norm,
               float clip_value, int first, void *ws, hipStream_t s) {
    double *partial = (double *)ws;
    float *coef = (float *)((char *)ws + kNormBlocks * sizeof(double));
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(kNormBlocks), dim3(256), 0, s, grad, trainable, n, partial);
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, s, partial, clip_norm, coef);
    hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, theta, grad, mom, trainable, n, lr, momentum, wd, coef,
                       clip_value, first);
    PF_LAUNCH_CHECK("sgd");
    return PF_OK;
}

}  // namespace pf
