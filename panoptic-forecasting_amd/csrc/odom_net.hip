// odometry forecaster (OdomModel.forward, models/odom/odom_model.py:79-106, shipped config) on gfx950.
//
// The network is nn.GRU(2, 128) + out = Linear(128, 2) on normalised [speed, yaw_rate]: T_in - 1 encoder steps from h = 0,
// then T_out decoder steps that feed their own output back (predict_type direct: current = y; offset: current += y).
// One launch runs a whole forecast: normalisation, every step, the head, the feedback and both output tensors.
//
// A workgroup (8 waves) owns a tile of R = 16*M sequences for the whole forecast.  Per step the hidden product
//   G[seq][col] = sum_k h[seq][k] * W_hh[col][k]      (384 columns = r, z, n rows of the 128 hidden units)
// runs on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation = the reference's precision): rows = sequences,
// wave w owns columns {r, z, n} x units w*16 .. w*16+15, so the gate epilogue has all three gates of a (sequence, unit) in
// one lane.  W_hh (196 608 B) is read once per workgroup and stays in registers for the whole forecast (96 floats per
// lane); h is double-buffered in LDS.  W_ih x (2 inputs) is VALU fmaf with the weights in registers.  The output head is
// a per-wave partial sum over the wave's 16 units (DPP butterfly inside the 16-lane row) followed by a fixed-order sum of
// the 8 wave partials in LDS.  Every step of a sequence sees the same instructions in the same order whatever M and
// wherever the sequence sits in its tile: MFMA rows never mix, so a sequence's outputs do not depend on the batch.
// Kernel nodes only (no memset / memcpy), no atomics: pf_odom_forward can be captured into a graph.
#include "odom_net.h"
#include "pf_prof.h"

namespace pf {
namespace odom {

// packed[((w*KS + ks)*3 + g)*64 + lane] = B operand of k-step ks, gate g, wave w:  W_hh[g*128 + w*16 + (lane&15)][k] with
// k = (ks>>2)*16 + (lane>>4)*4 + (ks&3), so that one ds_read_b128 of h[row][j*16 + (lane>>4)*4 ..] feeds k-steps 4j..4j+3
__global__ __launch_bounds__(256) void pack_whh_kernel(const float *__restrict__ whh, float *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= WAVES * KS * 3 * 64) return;
    const int lane = i & 63, g = (i >> 6) % 3, ks = (i / 192) % KS, w = i / (192 * KS);
    const int row = g * H + w * 16 + (lane & 15);
    const int k = (ks >> 2) * 16 + (lane >> 4) * 4 + (ks & 3);
    out[i] = whh[row * H + k];
}

__device__ __forceinline__ float sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// SAVE (training, odom_train.hip): the same instructions in the same order plus the stores of what the backward reads
template <int M, bool SAVE>
__global__ __launch_bounds__(THREADS) void odom_forward_kernel(Args a) {
#pragma clang fp contract(off)
    constexpr int R = 16 * M;
    __shared__ __attribute__((aligned(16))) float hb[2][R * HP];
    __shared__ float xin[T_MAX * R * 2];      // normalised inputs [t][row][2]
    __shared__ float part[WAVES * R * 2];     // head partials [wave][row][2]
    __shared__ float xcur[R * 2];             // decoder input [row][2]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int col = lane & 15, kg = lane >> 4;
    const int unit = wave * 16 + col;
    const long long b0 = (long long)blockIdx.x * R;
    const float *raw = a.raw;

    // W_hh for the whole forecast: 96 registers per lane
    float w[KS * 3];
    {
        const float *src = a.whh + (size_t)wave * KS * 3 * 64 + lane;
#pragma unroll
        for (int i = 0; i < KS * 3; ++i) w[i] = src[i * 64];
    }
    float wi[3][2], bi[3], bh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        wi[g][0] = raw[O_WIH + (g * H + unit) * 2];
        wi[g][1] = raw[O_WIH + (g * H + unit) * 2 + 1];
        bi[g] = raw[O_BIH + g * H + unit];
        bh[g] = raw[O_BHH + g * H + unit];
    }
    const float wo0 = raw[O_OUTW + unit], wo1 = raw[O_OUTW + H + unit];
    const float *mean = raw + O_MEAN, *stdv = raw + O_STD;

    for (int i = tid; i < a.T_in * R * 2; i += THREADS) {
        const int o = i & 1, row = (i >> 1) % R, t = i / (2 * R);
        const long long b = b0 + row;
        xin[i] = b < a.B ? (a.inps[(b * a.T_in + t) * 2 + o] - mean[o]) / stdv[o] : 0.f;
    }
    for (int i = tid; i < R * HP; i += THREADS) hb[0][i] = 0.f;
    float hold[M][4];
#pragma unroll
    for (int mt = 0; mt < M; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) hold[mt][r] = 0.f;
    __syncthreads();

    const int n_enc = a.T_in - 1, n_steps = n_enc + a.T_out;
    int p = 0;
    for (int s = 0; s < n_steps; ++s) {
        const bool dec = s >= n_enc;
        // decoder step 0 reads normalised inps[:, -1] (odom_model.py:88)
        const float *xs = dec ? (s == n_enc ? xin + (size_t)(a.T_in - 1) * R * 2 : xcur) : xin + (size_t)s * R * 2;
        f32x4 acc[M][3];
#pragma unroll
        for (int mt = 0; mt < M; ++mt)
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[mt][g] = f32x4{bh[g], bh[g], bh[g], bh[g]};
        const float *hcur = hb[p];
#pragma unroll
        for (int j = 0; j < KS / 4; ++j) {
#pragma unroll
            for (int mt = 0; mt < M; ++mt) {
                const f32x4 av = *reinterpret_cast<const f32x4 *>(hcur + (mt * 16 + col) * HP + j * 16 + kg * 4);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int g = 0; g < 3; ++g)
                        acc[mt][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], w[(4 * j + q) * 3 + g], acc[mt][g], 0, 0, 0);
            }
        }
        // gate epilogue (nn.GRU: r, z, n; b_hn inside r * (...)): lane holds rows kg*4 + r of each sub-tile, unit `unit`
        float *hnext = hb[p ^ 1];
        float y0[M][4], y1[M][4];
#pragma unroll
        for (int mt = 0; mt < M; ++mt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = mt * 16 + kg * 4 + r;
                const float x0 = xs[row * 2], x1 = xs[row * 2 + 1];
                const float ir = fmaf(wi[0][1], x1, fmaf(wi[0][0], x0, bi[0]));
                const float iz = fmaf(wi[1][1], x1, fmaf(wi[1][0], x0, bi[1]));
                const float in_ = fmaf(wi[2][1], x1, fmaf(wi[2][0], x0, bi[2]));
                const float rg = sigmoid(ir + acc[mt][0][r]);
                const float zg = sigmoid(iz + acc[mt][1][r]);
                const float ng = tanhf(in_ + rg * acc[mt][2][r]);
                const float hn = (1.f - zg) * ng + zg * hold[mt][r];
                hold[mt][r] = hn;
                hnext[row * HP + unit] = hn;
                if (SAVE && b0 + row < a.B) {
                    const size_t at = ((size_t)s * a.B + (size_t)(b0 + row)) * H + unit;
                    a.sv.h[at] = hn, a.sv.r[at] = rg, a.sv.z[at] = zg, a.sv.n[at] = ng, a.sv.q[at] = acc[mt][2][r];
                    if (wave == 0 && col < 2) a.sv.x[((size_t)s * a.B + (size_t)(b0 + row)) * 2 + col] = col ? x1 : x0;
                }
                y0[mt][r] = wo0 * hn;
                y1[mt][r] = wo1 * hn;
            }
        }
        if (dec) {
#pragma unroll
            for (int mt = 0; mt < M; ++mt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float s0 = row16_sum(y0[mt][r]), s1 = row16_sum(y1[mt][r]);
                    if (col == 0) {
                        const int row = mt * 16 + kg * 4 + r;
                        part[(wave * R + row) * 2] = s0;
                        part[(wave * R + row) * 2 + 1] = s1;
                    }
                }
            }
        }
        __syncthreads();
        if (dec) {
            if (tid < R * 2) {
                const int row = tid >> 1, o = tid & 1;
                float y = raw[O_OUTB + o];
#pragma unroll
                for (int v = 0; v < WAVES; ++v) y += part[(v * R + row) * 2 + o];
                const float cur = a.offset ? xs[tid] + y : y;
                xcur[tid] = cur;
                const long long b = b0 + row;
                if (b < a.B) {
                    const long long at = (b * a.T_out + (s - n_enc)) * 2 + o;
                    a.out_norm[at] = cur;
                    a.out[at] = cur * stdv[o] + mean[o];
                }
            }
            __syncthreads();
        }
        p ^= 1;
    }
}

int check_dims(int B, int T_in, int T_out, int flags) {
    if (flags & ~1) return fail(PF_EUNSUPPORTED, "pf_odom: unsupported flags 0x%x (bit 0 = predict_type offset)", flags);
    if (B < 0 || T_in < 2 || T_in > T_MAX || T_out < 1 || T_out > T_MAX)
        return fail(PF_EINVAL, "pf_odom: bad dims B=%d T_in=%d T_out=%d (B >= 0, 2 <= T_in <= %d, 1 <= T_out <= %d)", B, T_in,
                    T_out, T_MAX, T_MAX);
    return 0;
}

int cu_count(int *cus) {
    int dev = 0;
    PF_HIP_CHECK(hipGetDevice(&dev));
    PF_HIP_CHECK(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (*cus < 1) *cus = 1;
    return 0;
}

template <int M>
static int launch(const Args &a, hipStream_t s) {
    const int tiles = (a.B + 16 * M - 1) / (16 * M);
    const double steps = a.T_in - 1 + a.T_out;
    ProfScope ps(s, "pf::odom::odom_forward_kernel", 2.0 * a.B * steps * (G3 * (H + 2)) + 2.0 * a.B * a.T_out * 2 * H,
                 4.0 * a.B * (a.T_in + 4 * a.T_out) + 4.0 * tiles * G3 * H);
    hipLaunchKernelGGL((odom_forward_kernel<M, false>), dim3(tiles), dim3(THREADS), 0, s, a);
    PF_LAUNCH_CHECK("odom_forward_kernel");
    return 0;
}

template <int M>
static int launch_save(const Args &a, hipStream_t s) {
    const int tiles = (a.B + 16 * M - 1) / (16 * M);
    const double steps = a.T_in - 1 + a.T_out;
    ProfScope ps(s, "pf::odom::odom_train_forward_kernel", 2.0 * a.B * steps * (G3 * (H + 2)) + 2.0 * a.B * a.T_out * 2 * H,
                 4.0 * a.B * (a.T_in + 4 * a.T_out) + 4.0 * tiles * G3 * H + 4.0 * a.B * steps * (5 * H + 2));
    hipLaunchKernelGGL((odom_forward_kernel<M, true>), dim3(tiles), dim3(THREADS), 0, s, a);
    PF_LAUNCH_CHECK("odom_train_forward_kernel");
    return 0;
}

int launch_train_forward(const Args &a, int m, hipStream_t s) {
    switch (m) {
        case 1: return launch_save<1>(a, s);
        case 2: return launch_save<2>(a, s);
        default: return launch_save<3>(a, s);
    }
}

}  // namespace odom
}  // namespace pf

using namespace pf;
using namespace pf::odom;

extern "C" int pf_odom_weights_size(int flags, size_t *raw_floats, size_t *packed_floats) {
    if (!raw_floats || !packed_floats) return fail(PF_EINVAL, "pf_odom_weights_size: null output");
    if (int rc = check_dims(0, 2, 1, flags)) return rc;
    *raw_floats = RAW_TOTAL;
    *packed_floats = PACKED_TOTAL;
    return 0;
}

extern "C" int pf_odom_pack(const float *raw, float *packed, int flags, void *stream) {
    if (int rc = check_dims(0, 2, 1, flags)) return rc;
    if (!raw || !packed) return fail(PF_EINVAL, "pf_odom_pack: null buffer");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = launch_copy(packed, raw, RAW_TOTAL * sizeof(float), s)) return rc;
    hipLaunchKernelGGL(pack_whh_kernel, dim3((WAVES * KS * 3 * 64 + 255) / 256), dim3(256), 0, s, raw + O_WHH,
                       packed + PACKED_WHH);
    PF_LAUNCH_CHECK("pf_odom_pack");
    return 0;
}

extern "C" int pf_odom_forward(const float *packed, int flags, int B, int T_in, int T_out, const float *inps, float *out,
                               float *out_norm, void *stream) {
    if (int rc = check_dims(B, T_in, T_out, flags)) return rc;
    if (B == 0) return 0;      // nothing to forecast: no launch
    if (!packed || !inps || !out || !out_norm) return fail(PF_EINVAL, "pf_odom_forward: null buffer");
    int cus = 0;
    if (int rc = cu_count(&cus)) return rc;
    Args a;
    a.raw = packed;
    a.whh = packed + PACKED_WHH;
    a.inps = inps, a.out = out, a.out_norm = out_norm;
    a.B = B, a.T_in = T_in, a.T_out = T_out, a.offset = flags & 1;
    a.sv = Saved{};
    hipStream_t s = (hipStream_t)stream;
    switch (pick_m(B, cus)) {
        case 1: return launch<1>(a, s);
        case 2: return launch<2>(a, s);
        default: return launch<3>(a, s);
    }
}
