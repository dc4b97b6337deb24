// Train-mode BatchNorm of the bg training step - batch statistics, running-stat update, backward through ReLU + BN - and the
// bias gradient of the one convolution without BN, which shares the slab scheme.
#include "pf_prof.h"
#include "train_device.h"
#include "train_kernels.h"

namespace pf {

// partial[c][slab][k]: k = 0 sum(y), 1 sum(y^2)  (stats)   or   0 sum(g'), 1 sum(g' * xhat)  (backward)
constexpr int kBnSlabs = 64;
// the block's sums of v (all 256 threads call) -> partial[c][slab]
__device__ __forceinline__ void bn_block_partial(double (&v)[2], double *partial, int c, int slab) {
    block_reduce_d<2>(v);
    if (threadIdx.x != 0) return;
    partial[((long long)c * kBnSlabs + slab) * 2 + 0] = v[0];
    partial[((long long)c * kBnSlabs + slab) * 2 + 1] = v[1];
}

// y of an odd-width layer is the tiled convolution's own output: rows of Wp >= W floats (pad columns hold garbage and are never
// read).  Element p of plane (b, c) of a [..][H][W] tensor stored with row pitch Wp:
__device__ __forceinline__ long long pitched(long long plane, long long p, long long HW, int W, int Wp) {
    return W == Wp ? plane * HW + p : (plane * (HW / W) + p / W) * Wp + p % W;
}

// z = fma(y, sc, sh): (y - mean) * invstd * gamma + beta written as one scale/shift, like ATen's batch_norm CPU/CUDA transforms.
// The backward kernels redo exactly this from y, which they read anyway, to know where the ReLU cut - the stored activation is
// not read again (2 of the 7 tensor passes of a BatchNorm backward)
struct BnAffine { float sc, sh; };
__device__ __forceinline__ BnAffine bn_affine(float gamma, float beta, float mean, float invstd) {
    const float sc = gamma * invstd;
    return {sc, beta - mean * sc};
}
// one element of the backward pass: g' = g * [z > 0] and xhat.  g by pointer: it is loaded only where the ReLU let it through
struct BnPoint { float gp, xh; };
__device__ __forceinline__ BnPoint bn_point(const float *g, float y, float mean, float invstd, const BnAffine &a, int relu) {
    return {(!relu || __builtin_fmaf(y, a.sc, a.sh) > 0.f) ? *g : 0.f, (y - mean) * invstd};
}

__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float *y, int B, int C, long long HW, int W, int Wp, double *partial) {
    const int c = blockIdx.x, slab = blockIdx.y;
    double v[2] = {0.0, 0.0};
    const long long per = (long long)B * HW;
    for (long long i = (long long)slab * 256 + threadIdx.x; i < per; i += (long long)kBnSlabs * 256) {
        const long long b = i / HW, p = i - b * HW;
        const double x = (double)y[pitched((long long)b * C + c, p, HW, W, Wp)];
        v[0] += x;
        v[1] += x * x;
    }
    bn_block_partial(v, partial, c, slab);
}

// The second pass of a BatchNorm (forward: statistics -> scale / shift; backward: sums -> dy) needs the channel's 64 slab
// partials added up.  Every WAVE of the second-pass kernels does that itself - one partial pair per lane, a butterfly of
// shuffles (a fixed order: every wave gets the same bits) - instead of a tiny kernel between the passes: 138 launches of ~5 us
// fewer per training step, on the critical path of the backward chain.  One designated thread per channel (block x = 0 of
// sample 0) writes what the step keeps (mean / invstd / running statistics; dgamma / dbeta).
static_assert(kBnSlabs == 64, "one slab partial per lane");
__device__ __forceinline__ void bn_wave_sums(const double *partial, int c, double &s, double &q) {
    const double *p = partial + ((long long)c * kBnSlabs + (threadIdx.x & 63)) * 2;
    s = p[0];
    q = p[1];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        q += __shfl_xor(q, o);
    }
}
struct BnStats {        // forward statistics of one layer (kernel argument)
    const double *partial;
    double n;
    float eps, momentum;
    float *mean, *invstd, *running_mean, *running_var;   // running_*: null = leave them
};
// mean / invstd of the batch (+ running-stat update by the designated thread: nn.BatchNorm2d, momentum 0.1, unbiased variance
// in the running stat).  Called by all lanes of a wave
__device__ __forceinline__ void bn_finish_stats(const BnStats &st, int c, bool writer, float &mean_f, float &invstd_f) {
    double s, q;
    bn_wave_sums(st.partial, c, s, q);
    const double m = s / st.n;
    double var = q / st.n - m * m;
    var = var < 0.0 ? 0.0 : var;
    mean_f = (float)m;
    invstd_f = (float)(1.0 / sqrt(var + (double)st.eps));
    if (writer) {
        st.mean[c] = mean_f;
        st.invstd[c] = invstd_f;
        if (st.running_mean) {
            const double unbiased = st.n > 1.0 ? var * st.n / (st.n - 1.0) : var;
            st.running_mean[c] = (float)((1.0 - st.momentum) * (double)st.running_mean[c] + st.momentum * m);
            st.running_var[c] = (float)((1.0 - st.momentum) * (double)st.running_var[c] + st.momentum * unbiased);
        }
    }
}

// the channel's sums for the second backward pass (dbeta = sum g', dgamma = sum g' xhat, rounded to fp32 as the gradient arenas
// hold them); the designated thread adds them to the arenas (zeroed once per step)
__device__ __forceinline__ void bn_finish_bwd(const double *partial, int c, bool writer, float *dgamma, float *dbeta, float &s_f, float &q_f) {
    double s, q;
    bn_wave_sums(partial, c, s, q);
    s_f = (float)s;
    q_f = (float)q;
    if (writer) {
        dbeta[c] += s_f;
        dgamma[c] += q_f;
    }
}

// z = relu(gamma * (y - mean) * invstd + beta) into channel slice [choff, choff + C) of the destination tensor
__global__ __launch_bounds__(256) void bn_apply_relu_kernel(const float *y, BnStats st, const float *gamma,
                                                            const float *beta, int C, long long HW, int W, int Wp, float *dst, int dst_ctotal,
                                                            int dst_choff, int relu) {
    const int bc = blockIdx.y, b = bc / C, c = bc - b * C;
    const long long i4 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    float mean_c, invstd_c;
    bn_finish_stats(st, c, blockIdx.x == 0 && b == 0 && threadIdx.x == 0, mean_c, invstd_c);
    if (i4 >= HW) return;
    const BnAffine a = bn_affine(gamma[c], beta[c], mean_c, invstd_c);
    float *dp = dst + ((long long)b * dst_ctotal + dst_choff + c) * HW + i4;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i4 + k < HW) {
            float v = __builtin_fmaf(y[pitched(bc, i4 + k, HW, W, Wp)], a.sc, a.sh);
            dp[k] = relu ? fmaxf(v, 0.f) : v;
        }
}

// ---- the same four passes with 16-B accesses and no per-element index division (planes of HW % 4 == 0 elements): a block
// walks the planes of its channel sample by sample.  The statistics kernel widens each of its four values and sums x and x^2 in
// fp64, as the scalar kernel does: var = E[x^2] - mean^2 cancels, so with |mean| / std = R a quad's fp32 sum of squares (rounded
// at 2^-24 of mean^2) and its fp32 sum (an error d of the mean is 2 * mean * d of the variance) EACH put R^2 * 2^-24 of the variance
// into it (R = 300: 1e-3 of the running variance, 4e-4 of the activation; DESIGN.md, "Precision of the BatchNorm statistics").
// The backward kernel's quad sums are of g' and g' * xhat, both O(1) with no cancellation behind them: fp32 per quad, fp64 across
__global__ __launch_bounds__(256) void bn_stats_partial4_kernel(const float *y, int B, int C, int HW4, double *partial) {
    const int c = blockIdx.x, slab = blockIdx.y;
    double v[2] = {0.0, 0.0};
    for (int b = 0; b < B; ++b) {
        const tr_f32x4 *p = reinterpret_cast<const tr_f32x4 *>(y) + ((long long)b * C + c) * HW4;
        for (int i = slab * 256 + threadIdx.x; i < HW4; i += kBnSlabs * 256) {
            const tr_f32x4 x = p[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double xk = (double)x[k];
                v[0] += xk;
                v[1] = __builtin_fma(xk, xk, v[1]);
            }
        }
    }
    bn_block_partial(v, partial, c, slab);
}
__global__ __launch_bounds__(256) void bn_apply_relu4_kernel(const float *y, BnStats st, const float *gamma,
                                                             const float *beta, int C, int HW4, float *dst, int dst_ctotal, int dst_choff, int relu) {
    const int bc = blockIdx.y, b = bc / C, c = bc - b * C;
    const int i = blockIdx.x * 256 + threadIdx.x;
    float mean_c, invstd_c;
    bn_finish_stats(st, c, blockIdx.x == 0 && b == 0 && threadIdx.x == 0, mean_c, invstd_c);
    if (i >= HW4) return;
    const BnAffine a = bn_affine(gamma[c], beta[c], mean_c, invstd_c);
    tr_f32x4 v = reinterpret_cast<const tr_f32x4 *>(y)[(long long)bc * HW4 + i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = __builtin_fmaf(v[k], a.sc, a.sh);
        if (relu) v[k] = fmaxf(v[k], 0.f);
    }
    reinterpret_cast<tr_f32x4 *>(dst)[((long long)b * dst_ctotal + dst_choff + c) * HW4 + i] = v;
}

// backward through ReLU + BN:  g' = g * [z > 0];  dbeta = sum g';  dgamma = sum g' * xhat;
//                              dy = gamma * invstd * (g' - dbeta / N - xhat * dgamma / N)
__global__ __launch_bounds__(256) void bn_bwd_partial4_kernel(const float *g, const float *gamma, const float *beta, int t_ctotal, int choff,
                                                              const float *y, const float *mean, const float *invstd, int B, int C, int HW4,
                                                              int relu, double *partial) {
    const int c = blockIdx.x, slab = blockIdx.y;
    double v[2] = {0.0, 0.0};
    const float mu = mean[c], is = invstd[c];
    const BnAffine a = bn_affine(gamma[c], beta[c], mu, is);
    for (int b = 0; b < B; ++b) {
        const long long ti = ((long long)b * t_ctotal + choff + c) * HW4, yi = ((long long)b * C + c) * HW4;
        for (int i = slab * 256 + threadIdx.x; i < HW4; i += kBnSlabs * 256) {
            const tr_f32x4 g4 = reinterpret_cast<const tr_f32x4 *>(g)[ti + i], y4 = reinterpret_cast<const tr_f32x4 *>(y)[yi + i];
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float gk = g4[k];
                const BnPoint p = bn_point(&gk, y4[k], mu, is, a, relu);
                s0 += p.gp;
                s1 += p.gp * p.xh;
            }
            v[0] += (double)s0;
            v[1] += (double)s1;
        }
    }
    bn_block_partial(v, partial, c, slab);
}
// dy of this kernel multiplies by the sums divided once per thread, xh * (sum_gx / n); bn_dy_scalar below divides per element,
// (xh * sum_gx) / n.  The two round differently: a layer whose planes are dense and a multiple of 4 elements runs this form (every
// level of a crop whose width is a multiple of 128), the odd-width levels (50 and 25 pixels of an 800 x 800 crop) run the other
__global__ __launch_bounds__(256) void bn_bwd_apply4_kernel(const float *g, const float *beta, int t_ctotal, int choff, const float *y,
                                                            const float *mean, const float *invstd, const float *gamma, const double *partial,
                                                            float *dgamma, float *dbeta, int B, int C, int HW4, int relu, float *dy) {
    const int bc = blockIdx.y, b = bc / C, c = bc - b * C;
    const int i = blockIdx.x * 256 + threadIdx.x;
    float sum_g, sum_gx;
    bn_finish_bwd(partial, c, blockIdx.x == 0 && b == 0 && threadIdx.x == 0, dgamma, dbeta, sum_g, sum_gx);
    if (i >= HW4) return;
    const float n = (float)((double)B * 4.0 * (double)HW4);
    const long long ti = ((long long)b * t_ctotal + choff + c) * HW4 + i;
    const tr_f32x4 g4 = reinterpret_cast<const tr_f32x4 *>(g)[ti], y4 = reinterpret_cast<const tr_f32x4 *>(y)[(long long)bc * HW4 + i];
    const float mu = mean[c], is = invstd[c], ga = gamma[c], s0 = sum_g / n, s1 = sum_gx / n;
    const BnAffine a = bn_affine(ga, beta[c], mu, is);
    tr_f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float gk = g4[k];
        const BnPoint p = bn_point(&gk, y4[k], mu, is, a, relu);
        o[k] = ga * is * (p.gp - s0 - p.xh * s1);
    }
    reinterpret_cast<tr_f32x4 *>(dy)[(long long)bc * HW4 + i] = o;
}

int launch_bn_forward(const float *y, int B, int C, int H, int W, float eps, float momentum, const float *gamma, const float *beta,
                      float *running_mean, float *running_var, float *mean, float *invstd, double *partial, float *dst, int dst_ctotal,
                      int dst_choff, int relu, int y_pitch, hipStream_t s) {
    const long long HW = (long long)H * W;
    const int Wp = y_pitch > 0 ? y_pitch : W;
    const bool vec = (HW & 3) == 0 && HW / 4 < (1ll << 31) && Wp == W;
    // the label names the two kernels launched (tests assert the form by it); bytes: y read twice, dst written
    ProfScope ps(s, vec ? "bn_stats_partial4_kernel+bn_apply_relu4_kernel" : "bn_stats_partial_kernel+bn_apply_relu_kernel", 0.0,
                 4.0 * B * C * (double)HW * 3.0);
    if (vec) hipLaunchKernelGGL(bn_stats_partial4_kernel, dim3(C, kBnSlabs), dim3(256), 0, s, y, B, C, (int)(HW / 4), partial);
    else hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(C, kBnSlabs), dim3(256), 0, s, y, B, C, HW, W, Wp, partial);
    const BnStats st{partial, (double)B * HW, eps, momentum, mean, invstd, running_mean, running_var};
    if (vec)
        hipLaunchKernelGGL(bn_apply_relu4_kernel, dim3((unsigned)((HW / 4 + 255) / 256), B * C), dim3(256), 0, s, y, st, gamma, beta, C,
                           (int)(HW / 4), dst, dst_ctotal, dst_choff, relu);
    else
        hipLaunchKernelGGL(bn_apply_relu_kernel, dim3((unsigned)((HW / 4 + 256) / 256), B * C), dim3(256), 0, s, y, st, gamma, beta, C, HW,
                           W, Wp, dst, dst_ctotal, dst_choff, relu);
    PF_LAUNCH_CHECK("bn_forward");
    return PF_OK;
}
size_t bn_partial_doubles(int C) { return (size_t)C * kBnSlabs * 2; }

// ---- the scalar forms of the backward pass: any plane size, y optionally pitched
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const float *g, const float *gamma, const float *beta, int t_ctotal, int choff,
                                                             const float *y, const float *mean, const float *invstd, int B, int C, long long HW,
                                                             int W, int Wp, int relu, double *partial) {
    const int c = blockIdx.x, slab = blockIdx.y;
    double v[2] = {0.0, 0.0};
    const long long per = (long long)B * HW;
    const float mu = mean[c], is = invstd[c];
    const BnAffine a = bn_affine(gamma[c], beta[c], mu, is);
    for (long long i = (long long)slab * 256 + threadIdx.x; i < per; i += (long long)kBnSlabs * 256) {
        const long long b = i / HW, p = i - b * HW;
        const long long ti = ((long long)b * t_ctotal + choff + c) * HW + p;
        const BnPoint pt = bn_point(g + ti, y[pitched((long long)b * C + c, p, HW, W, Wp)], mu, is, a, relu);
        v[0] += (double)pt.gp;
        v[1] += (double)pt.gp * (double)pt.xh;
    }
    bn_block_partial(v, partial, c, slab);
}
// dy of the element g points to, whose y is yv: the sums divided per element (bn_bwd_apply4_kernel's comment)
__device__ __forceinline__ float bn_dy_scalar(const float *g, float yv, float gamma, float invstd, float beta, float mean, int relu, float sum_g,
                                              float sum_gx, float n) {
    const BnPoint p = bn_point(g, yv, mean, invstd, bn_affine(gamma, beta, mean, invstd), relu);
    return gamma * invstd * (p.gp - sum_g / n - p.xh * sum_gx / n);
}
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float *g, const float *beta, int t_ctotal, int choff, const float *y,
                                                           const float *mean, const float *invstd, const float *gamma, const double *partial,
                                                           float *dgamma, float *dbeta, int B, int C, long long HW, int relu, float *dy) {
    const int bc = blockIdx.y, b = bc / C, c = bc - b * C;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    float sum_g, sum_gx;
    bn_finish_bwd(partial, c, blockIdx.x == 0 && b == 0 && threadIdx.x == 0, dgamma, dbeta, sum_g, sum_gx);
    if (i >= HW) return;
    const float n = (float)((double)B * (double)HW);
    const long long ti = ((long long)b * t_ctotal + choff + c) * HW + i;
    dy[(long long)bc * HW + i] = bn_dy_scalar(g + ti, y[(long long)bc * HW + i], gamma[c], invstd[c], beta[c], mean[c], relu, sum_g, sum_gx, n);
}

// the same, dy written with a row pitch of Wp >= W floats and zeros in the pad columns: the layout the tiled convolutions of an
// odd-width level read (launch_pad_gather's, without the copy)
__global__ __launch_bounds__(256) void bn_bwd_apply_pitch_kernel(const float *g, const float *beta, int t_ctotal, int choff, const float *y,
                                                                 const float *mean, const float *invstd, const float *gamma, const double *partial,
                                                                 float *dgamma, float *dbeta, int B, int C, int H, int W, int Wp, int relu, int y_pitched,
                                                                 float *dy) {
    const int bc = blockIdx.y, b = bc / C, c = bc - b * C;
    const int ip = blockIdx.x * 256 + threadIdx.x;
    float sum_g, sum_gx;
    bn_finish_bwd(partial, c, blockIdx.x == 0 && b == 0 && threadIdx.x == 0, dgamma, dbeta, sum_g, sum_gx);
    if (ip >= H * Wp) return;
    const int yy = ip / Wp, x = ip - yy * Wp;
    float o = 0.f;
    if (x < W) {
        const long long HW = (long long)H * W, i = (long long)yy * W + x;
        const float n = (float)((double)B * (double)HW);
        const long long ti = ((long long)b * t_ctotal + choff + c) * HW + i;
        const float yv = y[y_pitched ? (long long)bc * H * Wp + ip : (long long)bc * HW + i];
        o = bn_dy_scalar(g + ti, yv, gamma[c], invstd[c], beta[c], mean[c], relu, sum_g, sum_gx, n);
    }
    dy[(long long)bc * H * Wp + ip] = o;
}

int launch_bn_backward(const float *g, int t_ctotal, int choff, const float *y, const float *mean, const float *invstd,
                       const float *gamma, const float *beta, int B, int C, int H, int W, int relu, float *dgamma, float *dbeta, double *partial, float *dy,
                       int dy_pitch, int y_pitch, hipStream_t s) {
    const long long HW = (long long)H * W;
    const int Wyp = y_pitch > 0 ? y_pitch : W;
    if (Wyp != W && dy_pitch != Wyp) return fail(PF_EINVAL, "bn_backward: a pitched y needs dy with the same pitch");
    const bool vec = (HW & 3) == 0 && HW / 4 < (1ll << 31) && Wyp == W;
    const bool pitch = dy_pitch > 0 && dy_pitch != W;
    // the label names the two kernels launched; bytes: g and y read twice, dy written
    const char *label = pitch ? (vec ? "bn_bwd_partial4_kernel+bn_bwd_apply_pitch_kernel" : "bn_bwd_partial_kernel+bn_bwd_apply_pitch_kernel")
                        : vec ? "bn_bwd_partial4_kernel+bn_bwd_apply4_kernel"
                              : "bn_bwd_partial_kernel+bn_bwd_apply_kernel";
    ProfScope ps(s, label, 0.0, 4.0 * B * C * (double)HW * 5.0);
    if (vec)
        hipLaunchKernelGGL(bn_bwd_partial4_kernel, dim3(C, kBnSlabs), dim3(256), 0, s, g, gamma, beta, t_ctotal, choff, y, mean, invstd, B, C,
                           (int)(HW / 4), relu, partial);
    else
        hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3(C, kBnSlabs), dim3(256), 0, s, g, gamma, beta, t_ctotal, choff, y, mean, invstd, B, C, HW, W, Wyp,
                           relu, partial);
    if (pitch)
        hipLaunchKernelGGL(bn_bwd_apply_pitch_kernel, dim3((unsigned)((H * dy_pitch + 255) / 256), B * C), dim3(256), 0, s, g, beta, t_ctotal, choff, y, mean,
                           invstd, gamma, partial, dgamma, dbeta, B, C, H, W, dy_pitch, relu, Wyp != W, dy);
    else if (vec)
        hipLaunchKernelGGL(bn_bwd_apply4_kernel, dim3((unsigned)((HW / 4 + 255) / 256), B * C), dim3(256), 0, s, g, beta, t_ctotal, choff, y, mean,
                           invstd, gamma, partial, dgamma, dbeta, B, C, (int)(HW / 4), relu, dy);
    else
        hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)((HW + 255) / 256), B * C), dim3(256), 0, s, g, beta, t_ctotal, choff, y, mean, invstd,
                           gamma, partial, dgamma, dbeta, B, C, HW, relu, dy);
    PF_LAUNCH_CHECK("bn_backward");
    return PF_OK;
}

// bias gradient of a conv without BN (finalConv): dbias[c] += sum over (b, pixels) of g; also copies g -> dy (contiguous).
// Grid (C, kBnSlabs) with fp64 partials reduced in slab order (one block per channel took 0.49 ms for the 11 logit planes)
__global__ __launch_bounds__(256) void bias_bwd_kernel(const float *g, int t_ctotal, int choff, int B, int C, long long HW, int W, int Wp,
                                                       double *partial, float *dy) {
    const int c = blockIdx.x, slab = blockIdx.y;
    double v[1] = {0.0};
    for (int b = 0; b < B; ++b) {
        const float *gp = g + ((long long)b * t_ctotal + choff + c) * HW;
        float *dp = dy + ((long long)b * C + c) * (HW / W) * Wp;      // rows of Wp >= W floats (pad columns: zeroed by the launcher)
        for (long long p = (long long)slab * 256 + threadIdx.x; p < HW; p += (long long)kBnSlabs * 256) {
            const float x = gp[p];
            dp[W == Wp ? p : (p / W) * Wp + p % W] = x;
            v[0] += (double)x;
        }
    }
    block_reduce_d<1>(v);
    if (threadIdx.x == 0) partial[(long long)c * kBnSlabs + slab] = v[0];
}
__global__ void bias_bwd_final_kernel(const double *partial, int C, float *dbias) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int k = 0; k < kBnSlabs; ++k) s += partial[(long long)c * kBnSlabs + k];
    dbias[c] += (float)s;
}
int launch_bias_backward(const float *g, int t_ctotal, int choff, int B, int C, int H, int W, float *dbias, double *partial, float *dy,
                         int dy_pitch, hipStream_t s) {
    const int Wp = dy_pitch > 0 ? dy_pitch : W;
    if (Wp != W) {
        int rc = launch_zero_fill(dy, (size_t)B * C * H * Wp * sizeof(float), s);
        if (rc) return rc;
    }
    ProfScope ps(s, "bias_bwd_kernel+bias_bwd_final_kernel", 0.0, 4.0 * B * C * (double)H * W * 2.0);
    hipLaunchKernelGGL(bias_bwd_kernel, dim3(C, kBnSlabs), dim3(256), 0, s, g, t_ctotal, choff, B, C, (long long)H * W, W, Wp, partial, dy);
    hipLaunchKernelGGL(bias_bwd_final_kernel, dim3((C + 63) / 64), dim3(64), 0, s, partial, C, dbias);
    PF_LAUNCH_CHECK("bias_bwd_kernel");
    return PF_OK;
}

}  // namespace pf
