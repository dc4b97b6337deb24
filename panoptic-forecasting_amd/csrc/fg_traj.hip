// fg forecaster: the small VALU kernels - instance feature model, trajectory GRU encoder / decoder with their output MLPs and
// normalisation, the gather of the selected step and the class row of the predictor - and their launchers.
#include "fg_net.h"
#include "pf_prof.h"

namespace pf {
namespace fg {

// _compute_traj_inst_feats (fg_model.py:206-214): relu(instance_compressor(x)) flattened channel-major -> instance_feat_model
// -> * mask.  One workgroup per (instance, step); x plane of step t at x + n*x_stride + t*t_stride.
__global__ __launch_bounds__(256) void inst_feat_kernel(const float *__restrict__ x, long long x_stride, long long t_stride,
                                                        const float *__restrict__ mask, int T, const float *__restrict__ wc,
                                                        const float *__restrict__ bc, const float *__restrict__ wf,
                                                        const float *__restrict__ bfv, float *__restrict__ out) {
    __shared__ float comp[ICC * HW];
    __shared__ float wcs[ICC * C];
    __shared__ float part[256];
    const int n = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const float *xp = x + n * x_stride + t * t_stride;
    for (int i = tid; i < ICC * C; i += 256) wcs[i] = wc[i];
    __syncthreads();
    if (tid < HW) {
        float s[ICC];
#pragma unroll
        for (int o = 0; o < ICC; ++o) s[o] = bc[o];
        for (int ci = 0; ci < C; ++ci) {
            const float v = xp[ci * HW + tid];
#pragma unroll
            for (int o = 0; o < ICC; ++o) s[o] = fmaf(wcs[o * C + ci], v, s[o]);
        }
#pragma unroll
        for (int o = 0; o < ICC; ++o) comp[o * HW + tid] = fmaxf(s[o], 0.f);
    }
    __syncthreads();
    const int o = tid >> 2, q = tid & 3;
    float s = 0.f;
    for (int i = q; i < ICC * HW; i += 4) s = fmaf(wf[o * ICC * HW + i], comp[i], s);
    part[tid] = s;
    __syncthreads();
    if (q == 0) {
        const float m = mask ? mask[n * T + t] : 1.f;
        out[((size_t)n * T + t) * IFH + o] = (part[tid] + part[tid + 1] + part[tid + 2] + part[tid + 3] + bfv[o]) * m;
    }
}

// One GRU step (nn.GRU, gate order r, z, n; b_hn inside r*(...)) for a workgroup of >= H threads: x[nin], h[H] in LDS;
// thread j < H returns h'_j.  Shared by the encoder and the decoder (and by any later GRU of the same form).
__device__ float gru_step(const float *x, int nin, const float *h, int H, const float *__restrict__ wih,
                          const float *__restrict__ whh, const float *__restrict__ bih, const float *__restrict__ bhh, int j) {
    float ir = bih[j], iz = bih[H + j], in_ = bih[2 * H + j];
    for (int k = 0; k < nin; ++k) {
        const float v = x[k];
        ir = fmaf(wih[(size_t)j * nin + k], v, ir);
        iz = fmaf(wih[(size_t)(H + j) * nin + k], v, iz);
        in_ = fmaf(wih[(size_t)(2 * H + j) * nin + k], v, in_);
    }
    float hr = bhh[j], hz = bhh[H + j], hn = bhh[2 * H + j];
    for (int k = 0; k < H; ++k) {
        const float v = h[k];
        hr = fmaf(whh[(size_t)j * H + k], v, hr);
        hz = fmaf(whh[(size_t)(H + j) * H + k], v, hz);
        hn = fmaf(whh[(size_t)(2 * H + j) * H + k], v, hn);
    }
    const float r = sigm(ir + hr), z = sigm(iz + hz);
    const float nn = tanhf(in_ + r * hn);
    return (1.f - z) * nn + z * h[j];
}

__device__ float dot_row(const float *__restrict__ w, const float *v, int n, float acc) {
    for (int k = 0; k < n; ++k) acc = fmaf(w[k], v[k], acc);
    return acc;
}

__device__ void traj_head(const TrajArgs &a, const float *h, float *hid, const float *prev, int slot, int n, int tid) {
    // traj_*_out (Linear, ReLU, Linear) of h, + prev (the residual current_traj + out, :309) when prev != nullptr
    hid[tid] = fmaxf(dot_row(a.w0 + tid * HID, h, HID, a.b0[tid]), 0.f);
    __syncthreads();
    if (tid < TR) {
        float v = dot_row(a.w2 + tid * HID, hid, HID, a.b2[tid]);
        if (prev) v += prev[tid];
        const size_t o = ((size_t)n * (1 + a.T_out) + slot) * TR + tid;
        a.traj_norm[o] = v;
        const float mean = tid < 8 ? a.traj_mean[tid] : a.depth_mean[tid - 8];
        const float sd = tid < 8 ? a.traj_std[tid] : a.depth_std[tid - 8];
        a.traj_unnorm[o] = v * sd + mean;
    }
}

// encoder (fg_model.py:236-275, 281): normalisation :167-204 + expand_traj_mask (model_utils.py:11-27), T_in GRU steps from
// h = 0, traj_feat_out of every step, traj_encoder_out of the last one
__global__ __launch_bounds__(HID) void traj_encoder_kernel(TrajArgs a) {
    __shared__ float xin[80], h[HID], hid[HID];
    const int n = blockIdx.x, tid = threadIdx.x;
    h[tid] = 0.f;
    for (int t = 0; t < a.T_in; ++t) {
        const int nt = n * a.T_in + t;
        if (tid < TR) {
            const float m = a.traj_mask[nt];
            const float dm = a.depth_mask[nt];
            float mk, v, mean, sd;
            if (tid < 4) mk = m;
            else if (tid < 8) mk = a.vel_mask[nt];
            else if (tid == 8) mk = dm;
            else mk = t > 0 ? dm * a.depth_mask[nt - 1] : 0.f;
            if (tid < 8) {
                v = a.trajs[nt * 8 + tid];
                mean = a.traj_mean[tid];
                sd = a.traj_std[tid];
            } else {
                v = a.depths[nt * 2 + tid - 8];
                mean = a.depth_mean[tid - 8];
                sd = a.depth_std[tid - 8];
            }
            xin[tid] = (v - mean) / sd * mk;
        } else if (tid < TR + IFH) {
            xin[tid] = a.instf[(size_t)nt * IFH + tid - TR];
        } else if (tid == TR + IFH) {
            xin[tid] = a.traj_mask[nt];
        } else if (tid < TR + IFH + 1 + OD) {
            const int k = tid - TR - IFH - 1;
            xin[tid] = (a.odom[((size_t)n * a.odom_T + t) * OD + k] - a.odom_mean[k]) / a.odom_std[k];
        }
        __syncthreads();
        const float hn = gru_step(xin, 80, h, HID, a.wih, a.whh, a.bih, a.bhh, tid);
        __syncthreads();
        h[tid] = hn;
        __syncthreads();
        if (tid < TF) a.tfeat[(size_t)nt * TF + tid] = dot_row(a.wtf + tid * HID, h, HID, a.btf[tid]);
    }
    a.gru_h[(size_t)n * HID + tid] = h[tid];
    traj_head(a, h, hid, nullptr, 0, n, tid);
}

// one decoder step (fg_model.py:289-309): input [current_traj, traj_inst_feats, out_odom[t]], GRU, current_traj + out,
// traj_feat_out of the new state (:295-296)
__global__ __launch_bounds__(HID) void traj_decoder_kernel(TrajArgs a) {
    __shared__ float xin[79], h[HID], hid[HID], cur[TR];
    const int n = blockIdx.x, tid = threadIdx.x, t = a.step;
    h[tid] = a.gru_h[(size_t)n * HID + tid];
    if (tid < TR) {
        cur[tid] = a.traj_norm[((size_t)n * (1 + a.T_out) + t) * TR + tid];
        xin[tid] = cur[tid];
    } else if (tid < TR + IFH) {
        xin[tid] = a.instf[(size_t)n * IFH + tid - TR];
    } else if (tid < TR + IFH + OD) {
        const int k = tid - TR - IFH;
        xin[tid] = (a.odom[((size_t)n * a.odom_T + a.T_in + t) * OD + k] - a.odom_mean[k]) / a.odom_std[k];
    }
    __syncthreads();
    const float hn = gru_step(xin, 79, h, HID, a.wih, a.whh, a.bih, a.bhh, tid);
    __syncthreads();
    h[tid] = hn;
    a.gru_h[(size_t)n * HID + tid] = hn;
    __syncthreads();
    if (tid < TF) a.tfeat[(size_t)n * TF + tid] = dot_row(a.wtf + tid * HID, h, HID, a.btf[tid]);
    traj_head(a, h, hid, cur, t + 1, n, tid);
}

// output_feats = mask_feats[:, -T_out:][range(N), output_inds] (:334); indices are clamped into [0, T_out)
__global__ __launch_bounds__(256) void gather_kernel(const float *__restrict__ mf, const int64_t *__restrict__ sel, int T_out,
                                                     float *__restrict__ out) {
    const int n = blockIdx.x;
    long long s = sel[n];
    s = s < 0 ? 0 : (s >= T_out ? T_out - 1 : s);
    const float4 *src = reinterpret_cast<const float4 *>(mf + ((size_t)n * (1 + T_out) + 1 + s) * C * HW);
    float4 *dst = reinterpret_cast<float4 *>(out + (size_t)n * C * HW);
    for (int i = threadIdx.x; i < C * HW / 4; i += 256) dst[i] = src[i];
}

// predictor row of each instance's class only (:335-336): masks[n] = W[cls] . y[n] + b[cls]; classes clamped into [0, 8)
__global__ __launch_bounds__(256) void predictor_kernel(const float *__restrict__ y, const int64_t *__restrict__ cls,
                                                        const float *__restrict__ w, const float *__restrict__ b,
                                                        float *__restrict__ out) {
    __shared__ float wr[C];
    const int n = blockIdx.x, tid = threadIdx.x;
    long long k = cls[n];
    k = k < 0 ? 0 : (k > 7 ? 7 : k);
    wr[tid] = w[k * C + tid];
    __syncthreads();
    const float *yn = y + (size_t)n * C * 784;
    for (int p = tid; p < 784; p += 256) {
        float s = b[k];
        for (int c = 0; c < C; ++c) s = fmaf(wr[c], yn[c * 784 + p], s);
        out[(size_t)n * 784 + p] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------- launchers
int launch_inst_feat(const float *x, long long x_stride, long long t_stride, const float *mask, int N, int T, const float *raw,
                     const Layout &L, float *out, const char *label, hipStream_t s) {
    ProfScope ps(s, label, 2.0 * N * T * (ICC * C * HW + IFH * ICC * HW), 4.0 * N * T * C * HW);
    hipLaunchKernelGGL(inst_feat_kernel, dim3(N, T), dim3(256), 0, s, x, x_stride, t_stride, mask, T, raw + L.raw[IC_W], raw + L.raw[IC_B],
                       raw + L.raw[IF_W], raw + L.raw[IF_B], out);
    PF_LAUNCH_CHECK("inst_feat_kernel");
    return 0;
}

int launch_traj(const TrajArgs &a, bool decoder, int N, const char *label, hipStream_t s) {
    ProfScope ps(s, label, decoder ? 2.0 * N * 3 * HID * (79 + HID) : 2.0 * N * a.T_in * 3 * HID * (80 + HID), 0);
    if (decoder) hipLaunchKernelGGL(traj_decoder_kernel, dim3(N), dim3(HID), 0, s, a);
    else hipLaunchKernelGGL(traj_encoder_kernel, dim3(N), dim3(HID), 0, s, a);
    PF_LAUNCH_CHECK(decoder ? "traj_decoder_kernel" : "traj_encoder_kernel");
    return 0;
}

int launch_gather(const float *mask_feats, const int64_t *sel, int N, int T_out, float *out, hipStream_t s) {
    hipLaunchKernelGGL(gather_kernel, dim3(N), dim3(256), 0, s, mask_feats, sel, T_out, out);
    PF_LAUNCH_CHECK("gather_kernel");
    return 0;
}

int launch_predictor(const float *y, const int64_t *cls, const float *w, const float *b, int N, float *out, const char *label, hipStream_t s) {
    ProfScope ps(s, label, 2.0 * N * 784 * C, 4.0 * N * 784 * C);
    hipLaunchKernelGGL(predictor_kernel, dim3(N), dim3(256), 0, s, y, cls, w, b, out);
    PF_LAUNCH_CHECK("predictor_kernel");
    return 0;
}

}  // namespace fg
}  // namespace pf
