// Convolution backward-weight on the fp32 matrix cores: the generic and the LDS-tiled kernel, their fixed-order reduction
// and the dispatch (the 3x3 stride-1 form with the taps folded into the matrix rows is wgrad_taps.hip).
#include "pf_prof.h"
#include "train_device.h"
#include "train_kernels.h"

namespace pf {

// dW[co][ci][tap] = sum over (b, oy, ox) of dy[b][co][oy][ox] * x[b][ci][oy*S + ky - P][ox*S + kx - P]
// GEMM on v_mfma_f32_16x16x4_f32: M = 16 couts, N = 16 cins, K = pixels (4 per instruction).  Workgroup = (cout tile,
// cin tile, slab of output rows); its 4 waves take the 16-pixel chunks of the slab's rows round-robin, keep the k*k
// tap accumulators in registers and are combined through LDS; partial sums go to partial[slab][co][ci][tap] and are
// added up by wgrad_reduce_kernel in slab order (no atomics: deterministic).
template <int KS, int STRIDE>
__global__ __launch_bounds__(256) void wgrad_partial_kernel(ConvArgs a, const float *dy, int B, int slabs, float *partial) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int KS2 = KS * KS, P = KS / 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int co = blockIdx.x * 16 + (lane & 15), ci = blockIdx.y * 16 + (lane & 15), kq = lane >> 4;
    const int slab = blockIdx.z;
    // this lane's input channel -> (source tensor, channel inside it)
    const float *xsrc = nullptr;
    long long xplane0 = 0;
    int x_ctotal = 0;
    if (ci < a.Cin) {
        int sidx = 0;
        while (sidx + 1 < a.n_src && ci >= a.src_cstart[sidx + 1]) ++sidx;
        xsrc = a.src[sidx];
        x_ctotal = a.src_ctotal[sidx];
        xplane0 = a.src_choff[sidx] + (ci - a.src_cstart[sidx]);
    }
    const long long in_plane = (long long)a.Hin * a.Win, out_plane = (long long)a.Hout * a.Wout;
    tr_f32x4 acc[KS2];
#pragma unroll
    for (int t = 0; t < KS2; ++t) acc[t] = tr_f32x4{0.f, 0.f, 0.f, 0.f};
    const int chunks_per_row = (a.Wout + 15) / 16;
    const long long rows = (long long)B * a.Hout;
    int work = 0;
    for (long long row = slab; row < rows; row += slabs) {
        const int b = (int)(row / a.Hout), oy = (int)(row - (long long)b * a.Hout);
        const float *dyp = (co < a.Cout) ? dy + ((long long)b * a.Cout + co) * out_plane + (long long)oy * a.Wout : nullptr;
        const float *xp = xsrc ? xsrc + ((long long)b * x_ctotal + xplane0) * in_plane : nullptr;
        for (int ch = 0; ch < chunks_per_row; ++ch, ++work) {
            if ((work & 3) != wave) continue;
            const int ox0 = ch * 16 + kq * 4;
            float av[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) av[j] = (dyp && ox0 + j < a.Wout) ? dyp[ox0 + j] : 0.f;
#pragma unroll
            for (int t = 0; t < KS2; ++t) {
                const int ky = t / KS, kx = t - ky * KS;
                const int iy = oy * STRIDE + ky - P;
                float bv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ix = (ox0 + j) * STRIDE + kx - P;
                    bv[j] = (xp && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win && ox0 + j < a.Wout) ? xp[(long long)iy * a.Win + ix] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc[t], 0, 0, 0);
            }
        }
    }
    // combine the 4 waves: D fragment = rows m = 4*(lane>>4)+i (cout), column n = lane&15 (cin)
    __shared__ float red[4][KS2][4][64];
#pragma unroll
    for (int t = 0; t < KS2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[wave][t][i][lane] = acc[t][i];
    __syncthreads();
    const int ci_pad = gridDim.y * 16, co_pad = gridDim.x * 16;
    for (int e = threadIdx.x; e < KS2 * 4 * 64; e += 256) {
        const int l = e & 63, i = (e >> 6) & 3, t = e >> 8;
        const float v = ((red[0][t][i][l] + red[1][t][i][l]) + red[2][t][i][l]) + red[3][t][i][l];
        const int m = blockIdx.x * 16 + 4 * (l >> 4) + i, n = blockIdx.y * 16 + (l & 15);
        partial[(((long long)slab * co_pad + m) * ci_pad + n) * KS2 + t] = v;
    }
#endif
}

// ---- the LDS-tiled form (input and output widths multiples of 4): round 2's kernel above gathered both operands
// straight from memory, 16 B per lane from 16 different planes per request, and every (cout tile, cin tile) pair
// re-read its operands: 12.8 TFLOP/s over the 70 layers of a B = 8, 800 x 800 step (tools/bench_train.py).  Here a
// workgroup owns 32 couts x 16 cins and walks 64-pixel row segments: dy [32][64] and the x rows the taps need
// [16][KS][64 S + 8] are loaded with coalesced 16-B loads one segment AHEAD (registers), parked in LDS, and the 4 waves
// multiply 16 pixels each for all k*k taps from there (pitches == 4 mod 32 floats: at most 2-way bank conflicts on
// the one-float-per-lane fragment reads).  Partial sums per slab as before, same fixed-order reduction.
// R = output rows per work item (round 4).  With R = 1 every x row is staged three times by a 3x3 layer (once per tap row of the
// three output rows it feeds); R = 2 stages KS + 1 rows for two output rows: 2 x rows per output row instead of 3, a fifth
// fewer bytes per multiply-add (the kernel is bound by its L2 -> LDS bytes)
template <int KS, int STRIDE, int R>
struct WgCfg {
    static constexpr int KS2 = KS * KS, P = KS / 2, TW = 64;
    static constexpr int XR = KS + (R - 1) * STRIDE;                // staged x rows
    static constexpr int XW = TW * STRIDE + 8;                      // staged x columns: [x0 S - 4, x0 S + 64 S + 4)
    static constexpr int XCP = (XR * XW + 27) / 32 * 32 + 4;        // channel pitch == 4 (mod 32), >= XR * XW
    static constexpr int DP = TW + 4;                               // dy row pitch: 68 == 4 (mod 32)
    static constexpr int NDY = R * 32 * (TW / 4), NX = 16 * XR * (XW / 4);   // float4 loads per item
    static constexpr int ITD = NDY / 256, ITX = (NX + 255) / 256;
    static constexpr int LDS_FLOATS = R * 32 * DP + 16 * XCP;
    static_assert(XCP >= XR * XW && XCP % 32 == 4 && NDY % 256 == 0, "wgrad tile geometry");
};

template <int KS, int STRIDE, int R>
__global__ __launch_bounds__(256) void wgrad_tiled_kernel(ConvArgs a, const float *dy, int B, int slabs, float *partial) {
#if defined(__HIP_DEVICE_COMPILE__)
    using C = WgCfg<KS, STRIDE, R>;
    __shared__ __attribute__((aligned(16))) float lds[C::LDS_FLOATS > 3 * 4 * 256 ? C::LDS_FLOATS : 3 * 4 * 256];
    float *dy_s = lds, *x_s = lds + R * 32 * C::DP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int co0 = blockIdx.x * 32, ci0 = blockIdx.y * 16, slab = blockIdx.z;
    const long long in_plane = (long long)a.Hin * a.Win, out_plane = (long long)a.Hout * a.Wout;
    const int chunks = (a.Wout + C::TW - 1) / C::TW;
    const int row_groups = (a.Hout + R - 1) / R;
    const long long items = (long long)B * row_groups * chunks;

    // this thread's x loads: (channel, tap row, 16-B column) of the staged window -> plane base of the channel (batch 0)
    const float *xplane[C::ITX];
    int xrow[C::ITX], xcol[C::ITX], xlds[C::ITX];
    int xbstride[C::ITX];   // channels of the tensor the plane lives in (batch stride in planes)
#pragma unroll
    for (int it = 0; it < C::ITX; ++it) {
        const int idx = it * 256 + tid;
        const int c = idx / (C::XR * (C::XW / 4)), r = idx - c * (C::XR * (C::XW / 4));
        const int row = r / (C::XW / 4), c4 = r - row * (C::XW / 4);
        const int ci = ci0 + c;
        xplane[it] = nullptr;
        xbstride[it] = 0;
        if (idx < C::NX && ci < a.Cin) {
            int sidx = 0;
            while (sidx + 1 < a.n_src && ci >= a.src_cstart[sidx + 1]) ++sidx;
            xplane[it] = a.src[sidx] + (long long)(a.src_choff[sidx] + (ci - a.src_cstart[sidx])) * in_plane;
            xbstride[it] = a.src_ctotal[sidx];
        }
        xrow[it] = row;
        xcol[it] = c4 * 4;
        xlds[it] = idx < C::NX ? c * C::XCP + row * C::XW + c4 * 4 : -1;
    }
    tr_f32x4 rdy[C::ITD], rx[C::ITX];
    auto fetch = [&](long long item) {
        const int ch = (int)(item % chunks);
        const long long row = item / chunks;
        const int b = (int)(row / row_groups), oy = (int)(row - (long long)b * row_groups) * R;
        const int x0 = ch * C::TW;
#pragma unroll
        for (int it = 0; it < C::ITD; ++it) {
            const int idx = it * 256 + tid, r2 = idx >> 9, c = (idx >> 4) & 31, c4 = idx & 15;
            const int co = co0 + c, ox = x0 + c4 * 4;
            rdy[it] = tr_f32x4{0.f, 0.f, 0.f, 0.f};
            if (co < a.Cout && ox < a.Wout && oy + r2 < a.Hout)   // Wout % 4 == 0: a 16-B piece is inside the row or outside it
                rdy[it] = *reinterpret_cast<const tr_f32x4 *>(dy + ((long long)b * a.Cout + co) * out_plane + (long long)(oy + r2) * a.Wout + ox);
        }
#pragma unroll
        for (int it = 0; it < C::ITX; ++it) {
            rx[it] = tr_f32x4{0.f, 0.f, 0.f, 0.f};
            const int iy = oy * STRIDE + xrow[it] - C::P, ix = x0 * STRIDE - 4 + xcol[it];
            if (xplane[it] && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win)
                rx[it] = *reinterpret_cast<const tr_f32x4 *>(xplane[it] + (long long)b * xbstride[it] * in_plane + (long long)iy * a.Win + ix);
        }
    };
    auto park = [&]() {
#pragma unroll
        for (int it = 0; it < C::ITD; ++it) {
            const int idx = it * 256 + tid;      // (row r2, cout c) = idx >> 4: rows of 32 couts follow each other
            *reinterpret_cast<tr_f32x4 *>(dy_s + (idx >> 4) * C::DP + (idx & 15) * 4) = rdy[it];
        }
#pragma unroll
        for (int it = 0; it < C::ITX; ++it)
            if (xlds[it] >= 0) *reinterpret_cast<tr_f32x4 *>(x_s + xlds[it]) = rx[it];
    };

    tr_f32x4 acc[2][C::KS2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int t = 0; t < C::KS2; ++t) acc[n][t] = tr_f32x4{0.f, 0.f, 0.f, 0.f};
    const int m = lane & 15, kq = lane >> 4;
    const bool two = co0 + 16 < a.Cout;   // the second cout tile exists (uniform)

    long long item = slab;
    if (item < items) fetch(item);
    for (; item < items; item += slabs) {
        __syncthreads();            // the previous segment has been multiplied
        park();
        __syncthreads();
        if (item + slabs < items) fetch(item + slabs);   // in flight during the MFMAs
#pragma unroll
        for (int r2 = 0; r2 < R; ++r2)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int q = wave * 4 + qq;                 // 4-pixel group of the segment
            const float a0 = dy_s[(r2 * 32 + m) * C::DP + q * 4 + kq];
            const float a1 = two ? dy_s[(r2 * 32 + 16 + m) * C::DP + q * 4 + kq] : 0.f;
#pragma unroll
            for (int t = 0; t < C::KS2; ++t) {
                const int ky = t / KS, kx = t - ky * KS;
                const float bv = x_s[m * C::XCP + (r2 * STRIDE + ky) * C::XW + (q * 4 + kq) * STRIDE + kx - C::P + 4];
                acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv, acc[0][t], 0, 0, 0);
                if (two) acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv, acc[1][t], 0, 0, 0);
            }
        }
    }
    // combine the 4 waves (3 taps per pass through LDS, fixed order) -> partial[slab][co][ci][tap]
    const int ci_pad = gridDim.y * 16, co_pad = gridDim.x * 32;
    float *red = lds;   // [3 taps][4 waves][256]
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int t0 = 0; t0 < C::KS2; t0 += 3) {
            __syncthreads();
#pragma unroll
            for (int tt = 0; tt < 3; ++tt)
                if (t0 + tt < C::KS2)
#pragma unroll
                    for (int i = 0; i < 4; ++i) red[(tt * 4 + wave) * 256 + i * 64 + lane] = acc[n][t0 + tt][i];
            __syncthreads();
            for (int e = tid; e < 3 * 256; e += 256) {
                const int tt = e >> 8, r = e & 255, i = r >> 6, l = r & 63;
                if (t0 + tt >= C::KS2) continue;
                const float v = ((red[(tt * 4 + 0) * 256 + r] + red[(tt * 4 + 1) * 256 + r]) + red[(tt * 4 + 2) * 256 + r]) + red[(tt * 4 + 3) * 256 + r];
                const int mm = co0 + n * 16 + 4 * (l >> 4) + i, nn = ci0 + (l & 15);
                partial[(((long long)slab * co_pad + mm) * ci_pad + nn) * C::KS2 + t0 + tt] = v;
            }
        }
#endif
}

// partial[slab][co_pad][ci_pad][ks2] -> dw[co][ci][tap] += sum over slabs.  A block = 64 consecutive outputs x 4 slab lanes:
// lane j adds the slabs j, j + 4, ... in order, the four sums are combined in fixed order through LDS (deterministic).  (As
// one thread per output walking all slabs this kernel was 5.7 ms of a 27 ms step: 90 blocks for a 91 -> 28 layer, each
// thread 341 dependent, strided loads.)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *partial, int slabs, int co_pad, int ci_pad, int ks2, int Cout, int Cin,
                                                           float *dw) {
    __shared__ float sm[4][64];
    const int j = threadIdx.x >> 6, l = threadIdx.x & 63;
    const long long o = (long long)blockIdx.x * 64 + l;
    const long long total = (long long)Cout * Cin * ks2;
    float s = 0.f;
    if (o < total) {
        const int t = (int)(o % ks2);
        const int ci = (int)((o / ks2) % Cin), co = (int)(o / ((long long)ks2 * Cin));
        const long long at = ((long long)co * ci_pad + ci) * ks2 + t, stride = (long long)co_pad * ci_pad * ks2;
        // four independent chains per lane (slabs k, k + 4, k + 8, k + 12 of its residue class): the loads of a chain are dependent
        // round trips to the L2, and a 91 -> 28 layer has 170 slabs; fixed order, so still bit-reproducible
        const float *p = partial + at;
        float s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int k = j;
        for (; k + 12 < slabs; k += 16) {
            s += p[k * stride];
            s1 += p[(k + 4) * stride];
            s2 += p[(k + 8) * stride];
            s3 += p[(k + 12) * stride];
        }
        for (; k < slabs; k += 4) s += p[k * stride];
        s = (s + s1) + (s2 + s3);
    }
    sm[j][l] = s;
    __syncthreads();
    if (j == 0 && o < total) dw[o] += ((sm[0][l] + sm[1][l]) + sm[2][l]) + sm[3][l];
}

static bool wgrad_tiled_ok(int Win, int Wout) { return (Win & 3) == 0 && (Wout & 3) == 0; }
// extents of partial[slab][co_pad][ci_pad][ks2]: whole cout tiles of 32 (the tiled and the folded-tap kernels: 2 tiles of 16 per
// workgroup) or 16 (wgrad_partial_kernel), whole cin tiles of 16
struct WgPad { int co, ci; };
static WgPad wgrad_pad(int cout, int cin, int co_tile) { return {(cout + co_tile - 1) / co_tile * co_tile, (cin + 15) / 16 * 16}; }

int wgrad_slabs(int cout, int cin, int ks, int B, int Hout, int Win, int Wout) {
    const bool tiled = wgrad_tiled_ok(Win, Wout);
    const long long tiles = (long long)(tiled ? (cout + 31) / 32 : (cout + 15) / 16) * ((cin + 15) / 16);
    // tiled: 512 workgroups per layer (2 per CU).  1024 gave each kernel more latency hiding alone, but twice the partial sums to
    // write and reduce, beside a backward chain that fills the other half of the chip anyway: 16.45 -> 16.2 ms per step (256: 17.9,
    // 384: 16.7, 768: 16.65 - same-box runs, profiles/r04_experiments.md)
    // (the 1x1 form - 15 KB of LDS, 58 registers, 8 workgroups per CU - wants the deeper queue: 2048, 15.65 -> 15.4 ms)
    long long s = (tiled ? (ks == 1 ? 2048 : 512) : 2048) / tiles;
    s = s < 1 ? 1 : s;
    const long long units = tiled ? (long long)B * Hout * ((Wout + 63) / 64) : (long long)B * Hout;
    return (int)(s > units ? units : s);
}
size_t wgrad_partial_floats(int cout, int cin, int ks, int B, int Hout, int Win, int Wout) {
    const WgPad pad = wgrad_pad(cout, cin, 32);      // covers the 16-wide form too
    return (size_t)wgrad_slabs(cout, cin, ks, B, Hout, Win, Wout) * pad.co * pad.ci * ks * ks;
}

int g_opt_wgrad_taps = 1;   // wgrad_taps: 3x3 stride-1 weight gradients with the taps folded into the matrix rows (wgrad_taps.hip)

// the instantiation for a layer (null: none is built); R = 2 where the tiled form has it
using WgKernel = void (*)(ConvArgs, const float *, int, int, float *);
static WgKernel wgrad_kernel(bool tiled, int ks, int stride) {
    if (ks == 3 && stride == 1) return tiled ? wgrad_tiled_kernel<3, 1, 2> : wgrad_partial_kernel<3, 1>;
    if (ks == 3 && stride == 2) return tiled ? wgrad_tiled_kernel<3, 2, 1> : wgrad_partial_kernel<3, 2>;
    if (ks == 1 && stride == 1) return tiled ? wgrad_tiled_kernel<1, 1, 1> : wgrad_partial_kernel<1, 1>;
    return nullptr;
}

int launch_wgrad(const ConvArgs &a, int ks, int stride, const float *dy, int B, float *partial, float *dw, hipStream_t s) {
    int slabs = wgrad_slabs(a.Cout, a.Cin, ks, B, a.Hout, a.Win, a.Wout);
    const bool tiled = wgrad_tiled_ok(a.Win, a.Wout);
    const bool taps = wgrad_taps_wanted(g_opt_wgrad_taps, ks, stride, a.Cin, a.Cout, a.Hin, a.Win, a.Hout, a.Wout);
    const WgPad pad = wgrad_pad(a.Cout, a.Cin, taps || tiled ? 32 : 16);
    if (taps) {
        if (int rc = launch_wgrad_taps(a, dy, B, slabs, pad.co, pad.ci, partial, &slabs, s)) return rc;      // (its profile scope carries the instantiation)
    } else {
        const WgKernel kernel = wgrad_kernel(tiled, ks, stride);
        if (!kernel) return fail(PF_EUNSUPPORTED, "wgrad: k=%d stride=%d", ks, stride);
        const bool two_rows = tiled && ks == 3 && stride == 1;      // R = 2: half as many work items (the partial buffer is sized for R = 1)
        if (two_rows) {
            const long long items2 = (long long)B * ((a.Hout + 1) / 2) * ((a.Wout + 63) / 64);
            slabs = (int)(slabs > items2 ? items2 : slabs);
        }
        char label[48];      // the instantiation, as the conv_dma labels name theirs: <KS, STRIDE, R> / <KS, STRIDE>
        if (tiled) snprintf(label, sizeof(label), "wgrad_tiled_kernel<%d, %d, %d>", ks, stride, two_rows ? 2 : 1);
        else snprintf(label, sizeof(label), "wgrad_partial_kernel<%d, %d>", ks, stride);
        ProfScope ps(s, label, 2.0 * B * a.Hout * a.Wout * (double)a.Cout * a.Cin * ks * ks,
                     4.0 * B * ((double)a.Cout * a.Hout * a.Wout + (double)a.Cin * a.Hin * a.Win));
        hipLaunchKernelGGL(kernel, dim3(pad.co / (tiled ? 32 : 16), pad.ci / 16, slabs), dim3(256), 0, s, a, dy, B, slabs, partial);
        PF_LAUNCH_CHECK("wgrad kernel");
    }
    const long long total = (long long)a.Cout * a.Cin * ks * ks;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, s, partial, slabs, pad.co, pad.ci, ks * ks, a.Cout, a.Cin, dw);
    PF_LAUNCH_CHECK("wgrad_reduce_kernel");
    return PF_OK;
}

}  // namespace pf
