// The output end of the bg network (HBM/L2-bound, VALU only):
//   head_kernel, head4_kernel, head_col_kernel<C> : final bilinear upsample + argmax   hardnet.py:372-384, bg_model.py:98
//   seg_loss_tile_kernel<C>, seg_loss_finish_kernel : the validation loss on the upsampled logits   bg_model.py:73-89
// net_select.cpp (choose_head, choose_seg_loss) says which of them a launch runs and with what grid and LDS size.
#include "net_kernels.h"
#include "conv_epilogue.h"
#include "pf_prof.h"

namespace pf {

// final upsample + argmax; logits [B,C,Hin,Win] -> seg [B,Hout,Wout] (+ optional full logits)
__global__ __launch_bounds__(256) void head_kernel(HeadArgs a) {
    const float sh = a.Hout > 1 ? (float)(a.Hin - 1) / (float)(a.Hout - 1) : 0.f;
    const float sw = a.Wout > 1 ? (float)(a.Win - 1) / (float)(a.Wout - 1) : 0.f;
    const size_t opl = (size_t)a.Hout * a.Wout, ipl = (size_t)a.Hin * a.Win;
    const size_t total = (size_t)a.B * opl;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int x = (int)(i % a.Wout);
        const size_t r = i / a.Wout;
        const int y = (int)(r % a.Hout);
        const int b = (int)(r / a.Hout);
        int y0, y1, x0, x1;
        float hy0, hy1, lx0, lx1;
        lin_coord(y, sh, a.Hin, y0, y1, hy0, hy1);
        lin_coord(x, sw, a.Win, x0, x1, lx0, lx1);
        const float *s = a.logits + (size_t)b * a.C * ipl;
        const size_t o00 = (size_t)y0 * a.Win + x0, o01 = (size_t)y0 * a.Win + x1;
        const size_t o10 = (size_t)y1 * a.Win + x0, o11 = (size_t)y1 * a.Win + x1;
        float best = -INFINITY;
        int arg = 0;
        for (int c = 0; c < a.C; ++c) {
            const float *sc = s + (size_t)c * ipl;
            const float t0 = lx0 * sc[o00] + lx1 * sc[o01];
            const float t1 = lx0 * sc[o10] + lx1 * sc[o11];
            const float v = hy0 * t0 + hy1 * t1;
            if (a.out_logits) a.out_logits[((size_t)b * a.C + c) * opl + (size_t)y * a.Wout + x] = v;
            if (v > best) { best = v; arg = c; }  // first maximum wins, like torch.argmax on CPU
        }
        if (a.out_is_i64) reinterpret_cast<long long *>(a.out_seg)[i] = arg;
        else reinterpret_cast<uint8_t *>(a.out_seg)[i] = (uint8_t)arg;
    }
}

// Fast path of the head for >= 3x upsampling (the bg net: logits at 1/4 resolution): one lane = 4 consecutive output
// pixels of a row.  Their taps fall on at most 3 consecutive source columns, so each channel costs 6 loads for 4
// outputs (the generic kernel: 16) and the labels leave as one 32-bit store.
__global__ __launch_bounds__(256) void head4_kernel(HeadArgs a) {
    const float sh = a.Hout > 1 ? (float)(a.Hin - 1) / (float)(a.Hout - 1) : 0.f;
    const float sw = a.Wout > 1 ? (float)(a.Win - 1) / (float)(a.Wout - 1) : 0.f;
    const size_t opl = (size_t)a.Hout * a.Wout, ipl = (size_t)a.Hin * a.Win;
    const int W4 = a.Wout >> 2;
    const size_t total = (size_t)a.B * a.Hout * W4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int xq = (int)(i % W4), x = xq * 4;
        const size_t r = i / W4;
        const int y = (int)(r % a.Hout), b = (int)(r / a.Hout);
        int y0, y1;
        float hy0, hy1;
        lin_coord(y, sh, a.Hin, y0, y1, hy0, hy1);
        int i0[4], i1[4];
        float l0[4], l1[4];
        int xa = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int x0, x1;
            lin_coord(x + k, sw, a.Win, x0, x1, l0[k], l1[k]);
            if (k == 0) xa = x0;
            i0[k] = x0 - xa;   // 0 or 1
            i1[k] = x1 - xa;   // 0, 1 or 2
        }
        const int xb = min(xa + 1, a.Win - 1), xc = min(xa + 2, a.Win - 1);
        const float *s = a.logits + (size_t)b * a.C * ipl;
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int arg[4] = {0, 0, 0, 0};
        for (int c = 0; c < a.C; ++c) {
            const float *r0 = s + (size_t)c * ipl + (size_t)y0 * a.Win, *r1 = s + (size_t)c * ipl + (size_t)y1 * a.Win;
            const float t0[3] = {r0[xa], r0[xb], r0[xc]}, t1[3] = {r1[xa], r1[xb], r1[xc]};
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float a0 = i0[k] ? t0[1] : t0[0], a1 = i1[k] == 2 ? t0[2] : (i1[k] ? t0[1] : t0[0]);
                const float b0 = i0[k] ? t1[1] : t1[0], b1 = i1[k] == 2 ? t1[2] : (i1[k] ? t1[1] : t1[0]);
                const float u0 = l0[k] * a0 + l1[k] * a1;
                const float u1 = l0[k] * b0 + l1[k] * b1;
                v[k] = hy0 * u0 + hy1 * u1;
                if (v[k] > best[k]) { best[k] = v[k]; arg[k] = c; }   // first maximum wins, like torch.argmax on CPU
            }
            if (a.out_logits)
                *reinterpret_cast<f32x4v *>(a.out_logits + ((size_t)b * a.C + c) * opl + (size_t)y * a.Wout + x) = f32x4v{v[0], v[1], v[2], v[3]};
        }
        const size_t o = (size_t)b * opl + (size_t)y * a.Wout + x;
        if (a.out_is_i64) {
            long long *d = reinterpret_cast<long long *>(a.out_seg) + o;
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = arg[k];
        } else {
            *reinterpret_cast<unsigned *>(reinterpret_cast<uint8_t *>(a.out_seg) + o) =
                (unsigned)arg[0] | ((unsigned)arg[1] << 8) | ((unsigned)arg[2] << 16) | ((unsigned)arg[3] << 24);
        }
    }
}

// Column head.  head4_kernel issues 6 scalar loads per channel per lane - 66 load instructions for 4 output pixels - and is
// bound by the texture addresser (188 us for 16 frames at 0.7 TB/s); a first tiled version (round 1: source window of a
// 16 x 256 output tile staged in LDS, a lane = 4 consecutive pixels of a row) removed the loads but left ~165 vector
// instructions per output pixel - per pixel and channel six selects of the 3 source columns its 4 pixels straddle, two
// horizontal and one vertical interpolation, the argmax update: 165 us, vector-ALU-bound (profiles/README.md).
// Here a lane owns ONE output column of a 32 x 256 tile and walks down its 32 rows:
//   * its two source columns and their weights are fixed: no selects;
//   * the horizontal interpolation of a source row (per channel: 2 LDS reads, mul, fma) is done once and serves the ~4
//     output rows between two source rows - the rows a lane needs are wave-uniform, so "next source row" is a scalar branch;
//   * per pixel and channel there remain the vertical interpolation (mul, fma) and the argmax update (compare, 2 selects);
//   * the per-row coordinates (lin_coord) are computed once per workgroup by 32 lanes and read back as LDS broadcasts.
// Same operations on the same values as head_kernel: u = lx0*a + lx1*b per source row, v = hy0*u0 + hy1*u1.
template <int CC>
__global__ __launch_bounds__(256) void head_col_kernel(HeadArgs a) {
    extern __shared__ float hl[];            // [CC][rows][cols] source window
    __shared__ int row_r0[kHeadCH], row_r1[kHeadCH];
    __shared__ float row_h1[kHeadCH];
    const float sh = a.Hout > 1 ? (float)(a.Hin - 1) / (float)(a.Hout - 1) : 0.f;
    const float sw = a.Wout > 1 ? (float)(a.Win - 1) / (float)(a.Wout - 1) : 0.f;
    const size_t opl = (size_t)a.Hout * a.Wout, ipl = (size_t)a.Hin * a.Win;
    const int ty0 = blockIdx.y * kHeadCH, tx0 = blockIdx.x * kHeadCW, b = blockIdx.z;
    const int ylast = min(ty0 + kHeadCH, a.Hout) - 1, xlast = min(tx0 + kHeadCW, a.Wout) - 1;
    const int sy0 = min((int)(sh * (float)ty0), a.Hin - 1), sx0 = min((int)(sw * (float)tx0), a.Win - 1);
    const int rows = min(min((int)(sh * (float)ylast), a.Hin - 1) + 1, a.Hin - 1) - sy0 + 1;
    const int cols = min(min((int)(sw * (float)xlast), a.Win - 1) + 1, a.Win - 1) - sx0 + 1;
    const int per = rows * cols;
    const float *src = a.logits + (size_t)b * CC * ipl;
    for (int e = threadIdx.x; e < per; e += 256) {
        const int r = e / cols, x = e - r * cols;
        const size_t off = (size_t)(sy0 + r) * a.Win + sx0 + x;
#pragma unroll
        for (int c = 0; c < CC; ++c) hl[c * per + e] = src[(size_t)c * ipl + off];
    }
    if (threadIdx.x < kHeadCH) {
        int y0, y1;
        float hy0, hy1;
        lin_coord(min(ty0 + (int)threadIdx.x, a.Hout - 1), sh, a.Hin, y0, y1, hy0, hy1);
        row_r0[threadIdx.x] = y0 - sy0;
        row_r1[threadIdx.x] = y1 - sy0;
        row_h1[threadIdx.x] = hy1;
    }
    __syncthreads();
    const int x = tx0 + threadIdx.x;
    if (x >= a.Wout) return;
    int x0, x1;
    float lx0, lx1;
    lin_coord(x, sw, a.Win, x0, x1, lx0, lx1);
    const float *p0 = hl + (x0 - sx0), *p1 = hl + (x1 - sx0);
    float tA[CC], tB[CC];                    // horizontally interpolated source rows curA (= y0) and curB (= y1)
    int curA = -1, curB = -1;                // wave-uniform
    auto hrow = [&](int r, float (&t)[CC]) {
#pragma unroll
        for (int c = 0; c < CC; ++c) t[c] = lx0 * p0[c * per + r * cols] + lx1 * p1[c * per + r * cols];
    };
    for (int ry = 0; ry < kHeadCH; ++ry) {
        const int y = ty0 + ry;
        if (y >= a.Hout) break;
        const int r0 = __builtin_amdgcn_readfirstlane(row_r0[ry]), r1 = __builtin_amdgcn_readfirstlane(row_r1[ry]);
        const float hy1 = row_h1[ry], hy0 = 1.f - hy1;
        if (r0 != curA) {
            if (r0 == curB) {
#pragma unroll
                for (int c = 0; c < CC; ++c) tA[c] = tB[c];
            } else {
                hrow(r0, tA);
            }
            curA = r0;
        }
        if (r1 != curB) {
            if (r1 == curA) {
#pragma unroll
                for (int c = 0; c < CC; ++c) tB[c] = tA[c];
            } else {
                hrow(r1, tB);
            }
            curB = r1;
        }
        float best = -INFINITY;
        int arg = 0;
        const size_t o = (size_t)b * opl + (size_t)y * a.Wout + x;
#pragma unroll
        for (int c = 0; c < CC; ++c) {
            const float v = hy0 * tA[c] + hy1 * tB[c];
            if (a.out_logits) a.out_logits[((size_t)b * CC + c) * opl + (size_t)y * a.Wout + x] = v;
            if (v > best) { best = v; arg = c; }   // first maximum wins, like torch.argmax on CPU
        }
        if (a.out_is_i64) reinterpret_cast<long long *>(a.out_seg)[o] = arg;
        else reinterpret_cast<uint8_t *>(a.out_seg)[o] = (uint8_t)arg;
    }
}

// ------------------------------------------------------------------------------------------------
// Validation loss of the bg model (scope row f4, forward part): BGModel.loss (bg_model.py:73-89) =
// nn.CrossEntropyLoss(ignore_index=255)(logits, labels) + accuracy, with logits = the bilinearly upsampled network output
// (hardnet.py:372-384).  Fused like the head: a workgroup stages the low-resolution logits of its 16 x 256 output tile in
// LDS, every lane interpolates the C logits of its pixels, forms log-sum-exp, the negative log-likelihood of the label
// and "argmax == label" - the full-resolution logits (92 MB per frame) are never written.  Per-workgroup partial sums
// (fp64) go to the workspace and a second one-block kernel adds them in index order: deterministic.
struct LossArgs {
    const float *logits;   // [B,C,Hin,Win]
    const void *labels;    // [B,Hout,Wout] i64 or u8
    double *partial;       // [blocks][3]: sum of nll, valid pixels, correct pixels
    int labels_i64, B, Hin, Win, Hout, Wout, ignore;
};

template <int CC>
__global__ __launch_bounds__(256) void seg_loss_tile_kernel(LossArgs a) {
    extern __shared__ float hl[];
    __shared__ double red[4][3];
    const float sh = a.Hout > 1 ? (float)(a.Hin - 1) / (float)(a.Hout - 1) : 0.f;
    const float sw = a.Wout > 1 ? (float)(a.Win - 1) / (float)(a.Wout - 1) : 0.f;
    const size_t opl = (size_t)a.Hout * a.Wout, ipl = (size_t)a.Hin * a.Win;
    // The staging of the source window is head_col_kernel's, written out a second time on purpose: moved into a shared inline function
    // (two forms tried: the arguments by reference, the scalars by value, either filling the caller's locals) hipcc orders the
    // instructions of all four tiled kernels differently and takes 1-2 more scalar registers, and their code is to stay as it is.
    const int ty0 = blockIdx.y * kHeadTH, tx0 = blockIdx.x * kHeadTW, b = blockIdx.z;
    const int ylast = min(ty0 + kHeadTH, a.Hout) - 1, xlast = min(tx0 + kHeadTW, a.Wout) - 1;
    const int sy0 = min((int)(sh * (float)ty0), a.Hin - 1), sx0 = min((int)(sw * (float)tx0), a.Win - 1);
    const int rows = min(min((int)(sh * (float)ylast), a.Hin - 1) + 1, a.Hin - 1) - sy0 + 1;
    const int cols = min(min((int)(sw * (float)xlast), a.Win - 1) + 1, a.Win - 1) - sx0 + 1;
    const int per = rows * cols;
    const float *src = a.logits + (size_t)b * CC * ipl;
    for (int e = threadIdx.x; e < per; e += 256) {
        const int r = e / cols, x = e - r * cols;
        const size_t off = (size_t)(sy0 + r) * a.Win + sx0 + x;
#pragma unroll
        for (int c = 0; c < CC; ++c) hl[c * per + e] = src[(size_t)c * ipl + off];
    }
    __syncthreads();
    double nll = 0.0, valid = 0.0, correct = 0.0;
    const int x = tx0 + threadIdx.x;
    if (x < a.Wout) {
        int x0, x1;
        float lx0, lx1;
        lin_coord(x, sw, a.Win, x0, x1, lx0, lx1);
        for (int ry = 0; ry < kHeadTH; ++ry) {
            const int y = ty0 + ry;
            if (y >= a.Hout) break;
            const size_t o = (size_t)b * opl + (size_t)y * a.Wout + x;
            const int lab = a.labels_i64 ? (int)reinterpret_cast<const long long *>(a.labels)[o] : (int)reinterpret_cast<const uint8_t *>(a.labels)[o];
            int y0, y1;
            float hy0, hy1;
            lin_coord(y, sh, a.Hin, y0, y1, hy0, hy1);
            const float *r0 = hl + (y0 - sy0) * cols - sx0, *r1 = hl + (y1 - sy0) * cols - sx0;
            float v[CC], best = -INFINITY;
            int arg = 0;
#pragma unroll
            for (int c = 0; c < CC; ++c) {
                const float t0 = lx0 * r0[c * per + x0] + lx1 * r0[c * per + x1];
                const float t1 = lx0 * r1[c * per + x0] + lx1 * r1[c * per + x1];
                v[c] = hy0 * t0 + hy1 * t1;
                if (v[c] > best) { best = v[c]; arg = c; }
            }
            if (lab == a.ignore || lab < 0 || lab >= CC) {
                // ignored pixel: no loss term, not in the accuracy denominator; a prediction never equals 255
                continue;
            }
            float se = 0.f, vl = 0.f;
#pragma unroll
            for (int c = 0; c < CC; ++c) {
                se += expf(v[c] - best);
                vl = c == lab ? v[c] : vl;
            }
            nll += (double)((best + logf(se)) - vl);
            valid += 1.0;
            correct += arg == lab ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nll += __shfl_xor(nll, o);
        valid += __shfl_xor(valid, o);
        correct += __shfl_xor(correct, o);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = nll; red[threadIdx.x >> 6][1] = valid; red[threadIdx.x >> 6][2] = correct;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *p = a.partial + ((size_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 3;
        p[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        p[1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        p[2] = ((red[0][2] + red[1][2]) + red[2][2]) + red[3][2];
    }
}

__global__ __launch_bounds__(256) void seg_loss_finish_kernel(const double *partial, int n, double *out3) {
    __shared__ double red[256][3];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) { s0 += partial[i * 3]; s1 += partial[i * 3 + 1]; s2 += partial[i * 3 + 2]; }
    red[threadIdx.x][0] = s0; red[threadIdx.x][1] = s1; red[threadIdx.x][2] = s2;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 256; ++i) { s0 += red[i][0]; s1 += red[i][1]; s2 += red[i][2]; }
        out3[0] = s0; out3[1] = s1; out3[2] = s2;
    }
}

// ------------------------------------------------------------------------------------------------
// launch a tiled kernel (head_col_kernel<C>, seg_loss_tile_kernel<C>); the instantiation's dynamic-LDS limit is raised on its first use
template <typename Args>
static int launch_tiled(void (*k)(Args), bool &raised, dim3 grid, size_t lds, hipStream_t s, const Args &a) {
    if (!raised) {
        PF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHeadLdsMax));
        raised = true;
    }
    hipLaunchKernelGGL(k, grid, dim3(kNetBlock), lds, s, a);
    return PF_OK;
}

int launch_head(const HeadArgs &a, hipStream_t s) {
    const HeadChoice c = choose_head(a);
    const double opx = (double)a.B * a.Hout * a.Wout;
    ProfScope ps(s, c.label, 0, 4.0 * a.B * a.C * a.Hin * a.Win + opx * (a.out_is_i64 ? 8 : 1) + (a.out_logits ? opx * a.C * 4 : 0));
    int rc = PF_OK;
    if (c.kind == HEAD_TILED) {
        switch (a.C) {
#define X(CC) case CC: { static bool raised = false; rc = launch_tiled(head_col_kernel<CC>, raised, c.grid, c.lds, s, a); break; }
            PF_HEAD_CLASSES(X)
#undef X
        }
    } else if (c.kind == HEAD_QUAD) {
        hipLaunchKernelGGL(head4_kernel, c.grid, dim3(kNetBlock), 0, s, a);
    } else {
        hipLaunchKernelGGL(head_kernel, c.grid, dim3(kNetBlock), 0, s, a);
    }
    if (rc) return rc;
    PF_LAUNCH_CHECK("head_kernel");
    return PF_OK;
}

}  // namespace pf

extern "C" int pf_seg_loss_workspace(int B, int out_h, int out_w, size_t *bytes) {
    if (!bytes || B <= 0 || out_h <= 0 || out_w <= 0) return pf::fail(PF_EINVAL, "pf_seg_loss_workspace: bad arguments");
    pf::LossChoice c{};
    pf::seg_loss_geometry(B, out_h, out_w, &c);
    *bytes = c.ws_bytes;
    return PF_OK;
}

extern "C" int pf_seg_loss(const float *logits, int B, int C, int Hin, int Win, const void *labels, int labels_i64, int out_h,
                           int out_w, int ignore_index, double *out3, void *ws, size_t ws_bytes, void *stream) {
    if (!logits || !labels || !out3 || !ws || B <= 0 || Hin <= 0 || Win <= 0 || out_h <= 0 || out_w <= 0)
        return pf::fail(PF_EINVAL, "pf_seg_loss: bad arguments");
    pf::LossChoice c{};
    const int refused = pf::choose_seg_loss(B, C, Hin, Win, out_h, out_w, &c);
    if (refused && !c.blocks) return refused;   // the class count
    // (a workspace too small is reported before a window too large, as it always was)
    if (ws_bytes < c.ws_bytes) return pf::fail(PF_EWORKSPACE, "pf_seg_loss: workspace %zu B < required %zu B", ws_bytes, c.ws_bytes);
    if (refused) return refused;
    pf::LossArgs a{logits, labels, (double *)ws, labels_i64 ? 1 : 0, B, Hin, Win, out_h, out_w, ignore_index};
    hipStream_t s = (hipStream_t)stream;
    {
        pf::ProfScope ps(s, c.label, 0.0, 4.0 * B * C * Hin * Win + (double)B * out_h * out_w * (labels_i64 ? 8 : 1));
        int rc = PF_OK;
        switch (C) {
#define X(CC) case CC: { static bool raised = false; rc = pf::launch_tiled(pf::seg_loss_tile_kernel<CC>, raised, c.grid, c.lds, s, a); break; }
            PF_HEAD_CLASSES(X)
#undef X
        }
        if (rc) return rc;
        PF_LAUNCH_CHECK("seg_loss_tile_kernel");
    }
    hipLaunchKernelGGL(pf::seg_loss_finish_kernel, dim3(1), dim3(256), 0, s, (const double *)ws, (int)c.blocks, out3);
    PF_LAUNCH_CHECK("seg_loss_finish_kernel");
    return PF_OK;
}
