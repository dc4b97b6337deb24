// odometry forecaster, training side (OdomModel.loss): the forward that keeps its gates and back-propagation through time.
//
// pf_odom_train_forward is odom_forward_kernel<M, SAVE = true> (odom_net.hip): the inference kernel's instructions in the
// inference kernel's order, plus the stores of h_s, r, z, n, q = W_hn h + b_hn and x_s per (step, sequence) into the
// workspace.  pf_odom_backward is three kernels:
//
//   odom_bptt_kernel<M>      mirrors the forward: a workgroup (8 waves) owns 16*M sequences for the whole reverse sweep,
//       W_hh^T (K = 384 gate rows -> 96 k-steps of v_mfma_f32_16x16x4_f32) stays in registers (wave w owns hidden units
//       16w .. 16w+15: 96 floats per lane), D_h = [da_r, da_z, dq] of the tile goes through LDS, dh stays in the lane that
//       holds the same (row, unit) as in the forward epilogue, dx = W_ih^T D_i is a row16_sum per wave + a fixed-order sum
//       of the 8 wave partials.  It overwrites the saved r, z, n, q with da_r, da_z, da_n, dq and writes gc (the gradient
//       of each decoder output) per (step, sequence).
//   odom_wgrad_kernel        every weight gradient is a sum over the S*B (step, sequence) rows: dW_hh [384 x 128] =
//       D_h^T h_{s-1} on the MFMA, db_hh, db_ih, dW_ih (D_i = [da_r, da_z, da_n] against x_s), dW_o, db_o (gc against
//       h_s) on the VALU from the same LDS chunk.  The rows are split into P contiguous ranges, one workgroup and one
//       partial (raw state_dict layout) each.
//   odom_wgrad_reduce_kernel grad_raw[i] = partial 0 + partial 1 + ... in that order; zeros in the odom_mean / odom_std slots.
//
// P depends on S*B only (never on the device), rows of a tile past B load zeros and so add exactly zero, and there is no
// atomic: two runs give the same bits.  Kernel nodes only.
#include "odom_net.h"
#include "pf_prof.h"

namespace pf {
namespace odom {

constexpr int DP = G3 + 4;         // LDS row stride of D_h in the sweep (b128 reads, as HP in the forward)
constexpr int CH = 16;             // (step, sequence) rows per LDS chunk of the weight-gradient kernel
constexpr int DS = G3 + 16;        // its row strides: 16 mod 64 banks, the 4 rows of a k-step land on distinct banks
constexpr int HS = H + 16;
constexpr int ROWS_PER_PART = 256; // rows per partial until P_MAX partials, then the ranges grow
constexpr int P_MAX = 256;

struct BArgs {
    const float *raw;
    Saved sv;
    const float *go, *gon;     // grad_out, grad_out_norm [B][T_out][2], either may be null
    int B, T_in, T_out, offset;
};

template <int M>
__global__ __launch_bounds__(THREADS) void odom_bptt_kernel(BArgs a) {
#pragma clang fp contract(off)
    constexpr int R = 16 * M;
    __shared__ __attribute__((aligned(16))) float dhs[R * DP];   // D_h of the tile [row][r | z | q]
    __shared__ float part[WAVES * R * 2];     // dx partials [wave][row][2]
    __shared__ float gcs[R * 2];              // gc of the decoder step after this one
    __shared__ float dxs[R * 2];              // dx of the step after this one
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int col = lane & 15, kg = lane >> 4;
    const int unit = wave * 16 + col;
    const long long b0 = (long long)blockIdx.x * R;
    const float *raw = a.raw;
    const size_t B = (size_t)a.B;

    // W_hh^T for the whole sweep: B operand of k-step i = W_hh[k][unit], k = (i>>2)*16 + kg*4 + (i&3) (one ds_read_b128
    // of D_h[row][j*16 + kg*4 ..] feeds k-steps 4j .. 4j+3)
    float w[G3 / 4];
#pragma unroll
    for (int i = 0; i < G3 / 4; ++i) w[i] = raw[O_WHH + ((i >> 2) * 16 + kg * 4 + (i & 3)) * H + unit];
    float wi[3][2];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        wi[g][0] = raw[O_WIH + (g * H + unit) * 2];
        wi[g][1] = raw[O_WIH + (g * H + unit) * 2 + 1];
    }
    const float wo0 = raw[O_OUTW + unit], wo1 = raw[O_OUTW + H + unit];
    const float *stdv = raw + O_STD;

    float dh[M][4];
#pragma unroll
    for (int mt = 0; mt < M; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dh[mt][r] = 0.f;
    if (tid < R * 2) gcs[tid] = 0.f, dxs[tid] = 0.f;
    __syncthreads();

    const int n_enc = a.T_in - 1, n_steps = n_enc + a.T_out;
    for (int s = n_steps - 1; s >= 0; --s) {
        const bool dec = s >= n_enc;
        const bool feeds = s > n_enc;         // x_s was the previous decoder step's output: its dx is wanted
        if (dec) {
            if (tid < R * 2) {
                const int row = tid >> 1, o = tid & 1, j = s - n_enc;
                const long long b = b0 + row;
                float g = 0.f;
                if (b < a.B) {
                    const size_t at = ((size_t)b * a.T_out + j) * 2 + o;
                    if (a.gon) g = a.gon[at];
                    if (a.go) g = g + stdv[o] * a.go[at];
                    if (j < a.T_out - 1) {
                        g = g + dxs[tid];
                        if (a.offset) g = g + gcs[tid];
                    }
                    a.sv.gc[((size_t)s * B + (size_t)b) * 2 + o] = g;
                }
                gcs[tid] = g;
            }
            __syncthreads();
        }
        float px0[M][4], px1[M][4];
#pragma unroll
        for (int mt = 0; mt < M; ++mt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = mt * 16 + kg * 4 + r;
                const bool valid = b0 + row < a.B;
                const size_t at = ((size_t)s * B + (size_t)(b0 + row)) * H + unit;
                float rg = 0.f, zg = 0.f, ng = 0.f, qg = 0.f, hp = 0.f;
                if (valid) {
                    rg = a.sv.r[at], zg = a.sv.z[at], ng = a.sv.n[at], qg = a.sv.q[at];
                    if (s > 0) hp = a.sv.h[at - B * H];
                }
                float d = dh[mt][r];
                if (dec) d = d + (wo0 * gcs[row * 2] + wo1 * gcs[row * 2 + 1]);
                const float dan = d * (1.f - zg) * (1.f - ng * ng);
                const float daz = d * (hp - ng) * (zg * (1.f - zg));
                const float dq = dan * rg;
                const float dar = dan * qg * (rg * (1.f - rg));
                dhs[row * DP + unit] = dar;
                dhs[row * DP + H + unit] = daz;
                dhs[row * DP + 2 * H + unit] = dq;
                if (valid) a.sv.r[at] = dar, a.sv.z[at] = daz, a.sv.n[at] = dan, a.sv.q[at] = dq;
                dh[mt][r] = d * zg;
                px0[mt][r] = wi[0][0] * dar + wi[1][0] * daz + wi[2][0] * dan;
                px1[mt][r] = wi[0][1] * dar + wi[1][1] * daz + wi[2][1] * dan;
            }
        }
        if (feeds) {
#pragma unroll
            for (int mt = 0; mt < M; ++mt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float s0 = row16_sum(px0[mt][r]), s1 = row16_sum(px1[mt][r]);
                    if (col == 0) {
                        const int row = mt * 16 + kg * 4 + r;
                        part[(wave * R + row) * 2] = s0;
                        part[(wave * R + row) * 2 + 1] = s1;
                    }
                }
            }
        }
        __syncthreads();
        // dh <- dh * z + W_hh^T D_h
        f32x4 acc[M];
#pragma unroll
        for (int mt = 0; mt < M; ++mt) acc[mt] = f32x4{dh[mt][0], dh[mt][1], dh[mt][2], dh[mt][3]};
#pragma unroll
        for (int j = 0; j < G3 / 16; ++j) {
#pragma unroll
            for (int mt = 0; mt < M; ++mt) {
                const f32x4 av = *reinterpret_cast<const f32x4 *>(dhs + (mt * 16 + col) * DP + j * 16 + kg * 4);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], w[4 * j + q], acc[mt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int mt = 0; mt < M; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) dh[mt][r] = acc[mt][r];
        if (feeds && tid < R * 2) {
            const int row = tid >> 1, o = tid & 1;
            float v = part[row * 2 + o];
#pragma unroll
            for (int u = 1; u < WAVES; ++u) v += part[(u * R + row) * 2 + o];
            dxs[tid] = v;
        }
        __syncthreads();
    }
}

struct WArgs {
    Saved sv;
    float *partials;           // [P][RAW_TOTAL]
    long long n_rows, rows_per_part, first_dec_row;
    long long B;
};

__global__ __launch_bounds__(THREADS) void odom_wgrad_kernel(WArgs a) {
    __shared__ float d_s[CH * DS];            // D_h [row][r | z | q]
    __shared__ float n_s[CH * HS];            // da_n
    __shared__ float hp_s[CH * HS];           // h_{s-1}
    __shared__ float hc_s[CH * HS];           // h_s
    __shared__ float x_s[CH * 2], gc_s[CH * 2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int col = lane & 15, kg = lane >> 4;
    f32x4 acc[G3 / 16];
#pragma unroll
    for (int t = 0; t < G3 / 16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float s_b0 = 0.f, s_b1 = 0.f, s_w0 = 0.f, s_w1 = 0.f;
    const long long row0 = (long long)blockIdx.x * a.rows_per_part;
    const long long row1 = row0 + a.rows_per_part < a.n_rows ? row0 + a.rows_per_part : a.n_rows;
    for (long long c = row0; c < row1; c += CH) {
        for (int i = tid; i < CH * H; i += THREADS) {
            const int rr = i >> 7, u = i & (H - 1);
            const long long row = c + rr;
            float vr = 0.f, vz = 0.f, vq = 0.f, vn = 0.f, vh = 0.f, vp = 0.f;
            if (row < row1) {
                const size_t at = (size_t)row * H + u;
                vr = a.sv.r[at], vz = a.sv.z[at], vq = a.sv.q[at], vn = a.sv.n[at], vh = a.sv.h[at];
                if (row >= a.B) vp = a.sv.h[at - (size_t)a.B * H];
            }
            d_s[rr * DS + u] = vr, d_s[rr * DS + H + u] = vz, d_s[rr * DS + 2 * H + u] = vq;
            n_s[rr * HS + u] = vn, hc_s[rr * HS + u] = vh, hp_s[rr * HS + u] = vp;
        }
        if (tid < CH * 2) {
            const long long row = c + (tid >> 1);
            const bool ok = row < row1;
            x_s[tid] = ok ? a.sv.x[(size_t)row * 2 + (tid & 1)] : 0.f;
            gc_s[tid] = ok && row >= a.first_dec_row ? a.sv.gc[(size_t)row * 2 + (tid & 1)] : 0.f;   // encoder steps have no head
        }
        __syncthreads();
        // dW_hh[t*16 + kg*4 + r][wave*16 + col] += sum over the chunk's rows of D_h[row][t*16 + ..] * h_{s-1}[row][wave*16 + col]
#pragma unroll
        for (int ks = 0; ks < CH / 4; ++ks) {
            const float bv = hp_s[(ks * 4 + kg) * HS + wave * 16 + col];
#pragma unroll
            for (int t = 0; t < G3 / 16; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(d_s[(ks * 4 + kg) * DS + t * 16 + col], bv, acc[t], 0, 0, 0);
        }
        if (tid < G3) {       // gate row tid: db_hh, db_ih, dW_ih
            for (int rr = 0; rr < CH; ++rr) {
                const float dv = d_s[rr * DS + tid];
                const float iv = tid >= 2 * H ? n_s[rr * HS + tid - 2 * H] : dv;
                s_b0 += dv, s_b1 += iv;
                s_w0 = fmaf(iv, x_s[rr * 2], s_w0), s_w1 = fmaf(iv, x_s[rr * 2 + 1], s_w1);
            }
        } else {              // hidden unit tid - 384: dW_o; units 0, 1 also db_o
            const int u = tid - G3;
            for (int rr = 0; rr < CH; ++rr) {
                const float hv = hc_s[rr * HS + u];
                s_w0 = fmaf(gc_s[rr * 2], hv, s_w0), s_w1 = fmaf(gc_s[rr * 2 + 1], hv, s_w1);
                if (u < 2) s_b0 += gc_s[rr * 2 + u];
            }
        }
        __syncthreads();
    }
    float *out = a.partials + (size_t)blockIdx.x * RAW_TOTAL;
#pragma unroll
    for (int t = 0; t < G3 / 16; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[O_WHH + (t * 16 + kg * 4 + r) * H + wave * 16 + col] = acc[t][r];
    if (tid < G3) {
        out[O_BHH + tid] = s_b0, out[O_BIH + tid] = s_b1;
        out[O_WIH + tid * 2] = s_w0, out[O_WIH + tid * 2 + 1] = s_w1;
    } else {
        const int u = tid - G3;
        out[O_OUTW + u] = s_w0, out[O_OUTW + H + u] = s_w1;
        if (u < 2) out[O_OUTB + u] = s_b0;
    }
}

__global__ __launch_bounds__(256) void odom_wgrad_reduce_kernel(const float *__restrict__ partials, int P, float *__restrict__ grad_raw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= RAW_TOTAL) return;
    float v = 0.f;
    if (i >= O_WIH)
        for (int p = 0; p < P; ++p) v += partials[(size_t)p * RAW_TOTAL + i];
    grad_raw[i] = v;
}

// the workspace: five [S*B][128] planes, x and gc [S*B][2], then the P partials
struct Layout {
    size_t rows, floats;
    int P;
    size_t rows_per_part;
};
static Layout layout(int B, int T_in, int T_out) {
    Layout l;
    l.rows = (size_t)B * (size_t)(T_in - 1 + T_out);
    size_t p = (l.rows + ROWS_PER_PART - 1) / ROWS_PER_PART;
    l.P = (int)(p < 1 ? 1 : (p > P_MAX ? P_MAX : p));
    l.rows_per_part = align_up((l.rows + l.P - 1) / l.P, CH);
    l.floats = l.rows * (5 * H + 4) + (size_t)l.P * RAW_TOTAL;
    return l;
}
static size_t ws_bytes_of(const Layout &l) { return align_up(l.floats * sizeof(float), 256); }
static Saved carve(void *ws, const Layout &l, float **partials) {
    float *p = (float *)ws;
    Saved s;
    s.h = p, s.r = p + l.rows * H, s.z = p + 2 * l.rows * H, s.n = p + 3 * l.rows * H, s.q = p + 4 * l.rows * H;
    s.x = p + 5 * l.rows * H, s.gc = s.x + 2 * l.rows;
    *partials = s.gc + 2 * l.rows;
    return s;
}

template <int M>
static int launch_bptt(const BArgs &a, hipStream_t s) {
    const int tiles = (a.B + 16 * M - 1) / (16 * M);
    const double steps = a.T_in - 1 + a.T_out;
    ProfScope ps(s, "pf::odom::odom_bptt_kernel", 2.0 * a.B * steps * (G3 * (H + 2)) + 2.0 * a.B * a.T_out * 2 * H,
                 4.0 * a.B * steps * (9 * H + 2) + 4.0 * tiles * G3 * H);
    hipLaunchKernelGGL((odom_bptt_kernel<M>), dim3(tiles), dim3(THREADS), 0, s, a);
    PF_LAUNCH_CHECK("odom_bptt_kernel");
    return 0;
}

static int launch_reduce(const float *partials, int P, float *grad_raw, hipStream_t s) {
    ProfScope ps(s, "pf::odom::odom_wgrad_reduce_kernel", (double)P * RAW_TOTAL, 4.0 * (P + 1) * RAW_TOTAL);
    hipLaunchKernelGGL(odom_wgrad_reduce_kernel, dim3((RAW_TOTAL + 255) / 256), dim3(256), 0, s, partials, P, grad_raw);
    PF_LAUNCH_CHECK("odom_wgrad_reduce_kernel");
    return 0;
}

}  // namespace odom
}  // namespace pf

using namespace pf;
using namespace pf::odom;

extern "C" int pf_odom_train_workspace(int B, int T_in, int T_out, int flags, size_t *bytes) {
    if (!bytes) return fail(PF_EINVAL, "pf_odom_train_workspace: null output");
    if (int rc = check_dims(B, T_in, T_out, flags)) return rc;
    *bytes = B == 0 ? 0 : ws_bytes_of(layout(B, T_in, T_out));
    return 0;
}

static int check_ws(const char *who, int B, int T_in, int T_out, const void *ws, size_t ws_bytes, Layout *l) {
    *l = layout(B, T_in, T_out);
    if (!ws) return fail(PF_EINVAL, "%s: null buffer", who);
    if (ws_bytes < ws_bytes_of(*l))
        return fail(PF_EINVAL, "%s: workspace of %zu bytes, pf_odom_train_workspace asks for %zu", who, ws_bytes, ws_bytes_of(*l));
    return 0;
}

extern "C" int pf_odom_train_forward(const float *packed, int flags, int B, int T_in, int T_out, const float *inps, float *out,
                                     float *out_norm, void *ws, size_t ws_bytes, void *stream) {
    if (int rc = check_dims(B, T_in, T_out, flags)) return rc;
    if (B == 0) return 0;
    if (!packed || !inps || !out || !out_norm) return fail(PF_EINVAL, "pf_odom_train_forward: null buffer");
    Layout l;
    if (int rc = check_ws("pf_odom_train_forward", B, T_in, T_out, ws, ws_bytes, &l)) return rc;
    int cus = 0;
    if (int rc = cu_count(&cus)) return rc;
    Args a;
    a.raw = packed;
    a.whh = packed + PACKED_WHH;
    a.inps = inps, a.out = out, a.out_norm = out_norm;
    a.B = B, a.T_in = T_in, a.T_out = T_out, a.offset = flags & 1;
    float *partials;
    a.sv = carve(ws, l, &partials);
    return launch_train_forward(a, pick_m(B, cus), (hipStream_t)stream);
}

extern "C" int pf_odom_backward(const float *packed, int flags, int B, int T_in, int T_out, const float *inps,
                                const float *out_norm, const float *grad_out, const float *grad_out_norm, void *ws,
                                size_t ws_bytes, float *grad_raw, void *stream) {
    if (int rc = check_dims(B, T_in, T_out, flags)) return rc;
    if (!grad_raw) return fail(PF_EINVAL, "pf_odom_backward: null buffer");
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) return launch_reduce(nullptr, 0, grad_raw, s);      // no sequence: the gradient is zero
    if (!packed || !inps || !out_norm) return fail(PF_EINVAL, "pf_odom_backward: null buffer");
    Layout l;
    if (int rc = check_ws("pf_odom_backward", B, T_in, T_out, ws, ws_bytes, &l)) return rc;
    int cus = 0;
    if (int rc = cu_count(&cus)) return rc;
    BArgs a;
    a.raw = packed;
    float *partials;
    a.sv = carve(ws, l, &partials);
    a.go = grad_out, a.gon = grad_out_norm;
    a.B = B, a.T_in = T_in, a.T_out = T_out, a.offset = flags & 1;
    int rc;
    switch (pick_m(B, cus)) {
        case 1: rc = launch_bptt<1>(a, s); break;
        case 2: rc = launch_bptt<2>(a, s); break;
        default: rc = launch_bptt<3>(a, s); break;
    }
    if (rc) return rc;
    WArgs wa;
    wa.sv = a.sv, wa.partials = partials;
    wa.n_rows = (long long)l.rows, wa.rows_per_part = (long long)l.rows_per_part;
    wa.first_dec_row = (long long)(T_in - 1) * B, wa.B = B;
    {
        ProfScope ps(s, "pf::odom::odom_wgrad_kernel", 2.0 * l.rows * (G3 * (H + 3) + 2 * H), 4.0 * l.rows * (6 * H + 4));
        hipLaunchKernelGGL(odom_wgrad_kernel, dim3(l.P), dim3(THREADS), 0, s, wa);
        PF_LAUNCH_CHECK("odom_wgrad_kernel");
    }
    return launch_reduce(partials, l.P, grad_raw, s);
}
