// The 1x1 packed-pair convolution (conv_s4.h: launch_s41_cfg; layout, operand split and weight stream: conv_mfma.h, conv_s4.hip).
#include <cstring>

#include "conv_s4.h"
#include "pf_prof.h"

namespace pf {

// 1x1: a streaming kernel (these layers are bound by their bytes: 2*Cin*Cout flops per pixel against 4*(Cin+Cout) bytes).
// One round = 8 group entries (32 channels); lane group g of an instruction supplies entries 2g and 2g+1.  The activation
// fragments come STRAIGHT from memory into registers - in the packed layout a 16-B load is [2 pixels][4 channels] of one
// term, which is the K-slice two M-tiles need (M-tile A = the even pixels of a 32-pixel row segment, M-tile B = the odd
// ones; 16 lanes x 16 B = 256 B contiguous per plane) - so there is no activation staging, and the only barrier per round
// is the one of the weight stages (LDS-DMA, double-buffered).  A wave owns rows 2w, 2w+1 of an 8x32-pixel tile and all NT
// cout tiles.  The D fragments of tiles A and B interleave to 8 consecutive pixels per lane, i.e. two of the 4-pixel
// fragments conv_epilogue.h works on (bias, upsampled residual, ReLU, 2x2 pool, fp32 or packed stores).
// The residual window of the tile (commuted upsample, conv_epilogue.h) is prefetched by 4-B LDS-DMA before the main loop.
template <int NT>
struct S41Cfg {
    static constexpr int TW = 32, TH = 8, MP = 4;
    static constexpr int WBUF = NT * 2 * 64 * 16;                   // [nt][term][lane][8 fp16]
    static constexpr int BIAS_OFF = 2 * WBUF;                       // the workgroup's bias values (DMA, read in the epilogue)
    static constexpr int MAIN = 2 * WBUF + 256;
    static constexpr int WPIECES = WBUF / 16, NITW = (WPIECES + 255) / 256;
};

typedef unsigned s4_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned s4_u32x2 __attribute__((ext_vector_type(2)));

template <int NT, int EPI>
__global__ __launch_bounds__(256, NT <= 2 ? 4 : (NT == 3 ? 3 : 2)) void conv_s4_1x1_kernel(ConvArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    using C = S41Cfg<NT>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int tid_lin, cgroup;   // XCD-aware order: the cout groups of a tile run back to back on one XCD and share its L2 (conv_mfma.h)
    xcd_tile_order(a.tilesX * a.tilesY, tid_lin, cgroup);
    const int tileY = tid_lin / a.tilesX, tileX = tid_lin - tileY * a.tilesX;
    const int tile0 = cgroup * NT, b = blockIdx.z;
    const size_t plane_bytes = (size_t)a.Hin * a.Win * 8;
    auto wbuf = [&](int i) { return smem_raw + i * C::WBUF; };
    const int g = lane >> 4;

    s4_f32x4 acc[C::MP][NT];
#pragma unroll
    for (int m = 0; m < C::MP; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = s4_f32x4{0.f, 0.f, 0.f, 0.f};
    const bool has_res = EPI == 1 && a.res && a.res_lds_off >= 0;
    ResWin rw = ResWin();

    // this lane's pixel pair in rows 2w, 2w+1: byte offset inside a group plane, or -1
    int poff[2];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int gy = tileY * C::TH + 2 * wave + rr, gx = tileX * C::TW + 2 * (lane & 15);
        poff[rr] = (gy < a.Hin && gx < a.Win) ? (gy * a.Win + gx) * 8 : -1;
    }
    unsigned woff[C::NITW];
#pragma unroll
    for (int it = 0; it < C::NITW; ++it) {
        const int p = it * 256 + tid, n = p / (2 * 64);
        woff[it] = (p < C::WPIECES && tile0 + n < a.ntiles) ? (unsigned)((tile0 + n) * a.nchunks * (2 * 64) + (p - n * (2 * 64))) * 16u : kS4Oob;
    }
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.wpk, 0, 0x7FFFFFFF, 0x00020000);

    // operand roles swapped (weights = A, pixels = B): lane (g, i) ends up with couts 4g..4g+3 of the pixel pair (2i, 2i+1).
    // Bias values through LDS (see conv_s4_kernel); zero for the low-resolution half of a commuted upsample (no_bias)
    float *bias_lds = reinterpret_cast<float *>(smem_raw + C::BIAS_OFF);
    if (wave == 0 && lane < NT * 16) {
        const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc((void *)a.bias, 0, 0x7FFFFFFF, 0x00020000);
        const int co = tile0 * 16 + lane;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(brs, (s4_lds_ptr_t)bias_lds, 4, (!a.no_bias && co < a.ntiles * 16) ? (unsigned)co * 4u : kS4Oob, 0,
                                                 0, 0);
    }

    const int cb = a.chunk_begin, nrounds = a.chunk_end - cb;
    // fragments of one round: [row][entry of the pair][term], each 16 B = 2 pixels x 4 channels
    auto load_round = [&](int r, s4_u32x4 (&x)[2][2][2]) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = 8 * (cb + r) + 2 * g + h;   // per lane group
            const char *hi;
            size_t tstride;
            const bool real = s4_entry_lane(a, e, b, plane_bytes, hi, tstride);   // padding entries (zero weights) read the zero page
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const bool ok = real && poff[rr] >= 0;
                const char *p = ok ? hi + poff[rr] : reinterpret_cast<const char *>(a.zero_page);
                x[rr][h][0] = *reinterpret_cast<const s4_u32x4 *>(p);
                x[rr][h][1] = *reinterpret_cast<const s4_u32x4 *>(ok ? p + tstride : p);
            }
        }
    };
    auto load_weights = [&](int r, unsigned char *wdst) {
#pragma unroll
        for (int it = 0; it < C::NITW; ++it)
            if (it * 256 + tid < C::WPIECES)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(wrsrc, (s4_lds_ptr_t)(wdst + (it * 256 + wave * 64) * 16), 16, woff[it],
                                                         (unsigned)(cb + r) * (2 * 64 * 16), 0, 0);
    };

    s4_u32x4 cur[2][2][2], nxt[2][2][2];
    if (nrounds > 0) {
        load_weights(0, wbuf(0));
        load_round(0, cur);
    }
    // residual window -> LDS, asynchronously, behind the first round's loads (fixed-size window of res_rows x res_cols per
    // channel, edge-clamped)
    if (has_res) {
        rw = res_window(a, tileY * C::TH, C::TH, tileX * C::TW, C::TW);
        rw.rows = a.res_rows;
        rw.cols = a.res_cols;
        rw.cs = res_chan_stride(a.res_rows, a.res_cols);
        const unsigned per = (unsigned)(rw.rows * rw.cols), total = (unsigned)(NT * 16 * rw.cs);
        const size_t rplane = (size_t)a.Hres * a.Wres;
        const __amdgpu_buffer_rsrc_t rrs = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(a.res + ((size_t)b * a.res_ctotal + a.res_choff + tile0 * 16) * rplane), 0, 0x7FFFFFFF, 0x00020000);
        unsigned char *rdst = smem_raw + a.res_lds_off * 4;
        for (unsigned e0 = (unsigned)wave * 64; e0 < total; e0 += 256) {
            const unsigned e = e0 + lane;
            const unsigned c = __umulhi(e, a.res_magic_cs), rem = e - c * (unsigned)rw.cs;
            const unsigned r = __umulhi(rem, a.res_magic_cols), x = rem - r * (unsigned)rw.cols;
            const int row = min(rw.sy0 + (int)r, a.Hres - 1), col = min(rw.sx0 + (int)x, a.Wres - 1);
            const bool ok = e < total && rem < per && tile0 * 16 + (int)c < a.Cout;
            const unsigned off = ok ? (unsigned)((c * rplane + (size_t)row * a.Wres + col) * 4) : kS4Oob;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rrs, (s4_lds_ptr_t)(rdst + e0 * 4), 4, off, 0, 0, 0);
        }
    }

    for (int round = 0; round < nrounds; ++round) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // weights of this round (and everything older) have landed
        __syncthreads();
        const bool more = round + 1 < nrounds;
        if (more) {
            load_weights(round + 1, wbuf((round + 1) & 1));
            load_round(round + 1, nxt);
        }
        const unsigned char *wb = wbuf(round & 1);
        s4_h8 bh[NT], bm[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            bh[n] = *reinterpret_cast<const s4_h8 *>(wb + ((n * 2 + 0) * 64 + lane) * 16);
            bm[n] = *reinterpret_cast<const s4_h8 *>(wb + ((n * 2 + 1) * 64 + lane) * 16);
        }
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int q = 0; q < 2; ++q) {   // q = pixel parity: low / high 8 B of the loads
                const s4_u32x4 h0 = cur[rr][0][0], h1 = cur[rr][1][0], m0 = cur[rr][0][1], m1 = cur[rr][1][1];
                const s4_u32x4 fh = q ? s4_u32x4{h0[2], h0[3], h1[2], h1[3]} : s4_u32x4{h0[0], h0[1], h1[0], h1[1]};
                const s4_u32x4 fm = q ? s4_u32x4{m0[2], m0[3], m1[2], m1[3]} : s4_u32x4{m0[0], m0[1], m1[0], m1[1]};
                const s4_h8 ah = __builtin_bit_cast(s4_h8, fh), am = __builtin_bit_cast(s4_h8, fm);
                const int m = rr * 2 + q;
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[m][n] = PF_MFMA_SPLIT(bh[n], am, acc[m][n]);
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[m][n] = PF_MFMA_SPLIT(bm[n], ah, acc[m][n]);
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[m][n] = PF_MFMA_SPLIT(bh[n], ah, acc[m][n]);
            }
        if (more) {
#pragma unroll
            for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int t = 0; t < 2; ++t) cur[rr][h][t] = nxt[rr][h][t];
        }
    }

    // ---- epilogue, lane-local: acc[rr*2 + q][n][r] = cout (tile0+n)*16 + 4g + r at pixel (row 2w + rr, column x0 + 2i + q).
    //      bias -> (+ bilinearly upsampled residual) -> ReLU -> (2x2 average pool: the pixel pair of a lane and its two rows)
    //      -> one [2 px][4 ch] unit per term (16 lanes = 256 B contiguous), [1 px][4 ch] when pooled, or fp32 NCHW pairs
    if (has_res) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();   // every wave's pieces of the residual window have landed
    }
    {
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) the compiler can see: no waits for loads inside the store loop (conv_s4_kernel)
        const lds_float *res_lds = (const lds_float *)(reinterpret_cast<float *>(smem_raw) + (has_res ? a.res_lds_off : 0));
        const int i2 = 2 * (lane & 15);
        const int ox = tileX * C::TW + i2;
        const bool pooled = EPI == 1 && a.pool;
        const int Ho = pooled ? a.Hout >> 1 : a.Hout, Wo = pooled ? a.Wout >> 1 : a.Wout;
        const size_t hw = (size_t)Ho * Wo;
        const S4Dst sd = s4_dst(a, b, hw);   // (conv_epilogue.h: s4_store_px)
        float vmax = 0.f;   // range guard of the operand split (conv_mfma.h)
        const float relu_lo1 = a.relu ? 0.f : -__builtin_inff();
        // finished values of pixel (rr, q), cout tile n
        auto finish = [&](int rr, int q, int n, const int (&o0)[2], const int (&o1)[2], const float (&lx1)[2], float hy1) {
            s4_f32x4 v = acc[rr * 2 + q][n];
            const s4_f32x4 b4 = *reinterpret_cast<const s4_f32x4 *>(bias_lds + n * 16 + 4 * g);
            // s4_finish (conv_epilogue.h) with the residual between the bias and the max, written out in one loop: with the two cases in
            // branches of their own the compiler contracted the residual's sums with the bias step differently and the +res launches
            // stored other bits (cu and c7 of tools/dump_s4_planes.py; profiles/s4_store_unify.md)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = v[r] * a.acc_scale + b4[r];   // acc_scale = 2^-k of the weight scaling: exact
                if (has_res) {   // same arithmetic as res_apply (conv_epilogue.h)
                    const lds_float *chan = res_lds + (n * 16 + 4 * g + r) * rw.cs;
                    const float lx0 = 1.f - lx1[q], hy0 = 1.f - hy1;
                    const float t0 = lx0 * chan[o0[q]] + lx1[q] * chan[o0[q] + 1];
                    const float t1 = lx0 * chan[o1[q]] + lx1[q] * chan[o1[q] + 1];
                    v[r] += hy0 * t0 + hy1 * t1;
                }
                v[r] = fmaxf(v[r], relu_lo1);
            }
            vmax = range_acc(vmax, v[0], v[1], v[2], v[3]);
            return v;
        };
        // store 4 channels (couts co..co+3) of ONE output pixel at element offset pix
        auto store_px = [&](int co, size_t pix, s4_f32x4 v) {
            if (a.dst_fmt) {
                s4_store_px(sd, co, pix, v);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (co + r < a.Cout) a.dst[((size_t)b * a.dst_ctotal + a.dst_choff + co + r) * hw + pix] = v[r];
            }
        };
        // ... and of the PAIR of pixels (pix, pix + 1): one 16-B unit per term when the group is whole
        auto store_pair = [&](int co, size_t pix, s4_f32x4 v0, s4_f32x4 v1) {
            const int chb = a.dst_choff + co;
            if (a.dst_fmt && (sd.choff & 2) == 0 && chb + 2 < sd.limit) {   // s4_store_px's whole-group case for two pixels
                s4_h4 h0, m0, h1, m1;
                split_terms4(v0, h0, m0);
                split_terms4(v1, h1, m1);
                const s4_h8 hi = s4_join(h0, h1), mid = s4_join(m0, m1);
                char *p = sd.base + pix * 8 + (size_t)(chb >> 2) * sd.hw * 8;
                *reinterpret_cast<s4_h8 *>(p) = hi;
                *reinterpret_cast<s4_h8 *>(p + sd.term) = mid;
            } else if (!a.dst_fmt) {
                typedef float f2 __attribute__((ext_vector_type(2)));
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (co + r < a.Cout)
                        *reinterpret_cast<f2 *>(a.dst + ((size_t)b * a.dst_ctotal + a.dst_choff + co + r) * hw + pix) = f2{v0[r], v1[r]};
            } else {
                store_px(co, pix, v0);
                store_px(co, pix + 1, v1);
            }
        };
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            if (pooled && rr == 1) continue;   // row 2w+1 is consumed with row 2w
            const int oy = tileY * C::TH + 2 * wave + rr;
            if (oy >= a.Hout || ox >= a.Wout) continue;
            if (pooled && oy + 1 >= a.Hout) continue;
            // interpolation taps of the two pixels (rows oy and, pooled, oy + 1)
            int o0[2] = {0, 0}, o1[2] = {0, 0}, p0[2] = {0, 0}, p1[2] = {0, 0};
            float lx1[2] = {0.f, 0.f}, hy1 = 0.f, hy1b = 0.f;
            if (has_res) {
                int y0, y1;
                float hy0;
                lin_coord(oy, a.res_sh, a.Hres, y0, y1, hy0, hy1);
                int z0 = 0, z1 = 0;
                if (pooled) lin_coord(oy + 1, a.res_sh, a.Hres, z0, z1, hy0, hy1b);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    int x0, x1;
                    float lx0;
                    lin_coord(min(ox + q, a.Wout - 1), a.res_sw, a.Wres, x0, x1, lx0, lx1[q]);
                    o0[q] = (y0 - rw.sy0) * rw.cols + (x0 - rw.sx0);
                    o1[q] = (y1 - rw.sy0) * rw.cols + (x0 - rw.sx0);
                    p0[q] = (z0 - rw.sy0) * rw.cols + (x0 - rw.sx0);
                    p1[q] = (z1 - rw.sy0) * rw.cols + (x0 - rw.sx0);
                }
            }
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int co = (tile0 + n) * 16 + 4 * g;
                if (co >= a.Cout + 2) continue;   // nothing of this unit is stored (dst_limit <= Cout + 2)
                const s4_f32x4 va = finish(rr, 0, n, o0, o1, lx1, hy1), vb = finish(rr, 1, n, o0, o1, lx1, hy1);
                if (!pooled) {
                    store_pair(co, (size_t)oy * a.Wout + ox, va, vb);
                } else {
                    const s4_f32x4 vc = finish(1, 0, n, p0, p1, lx1, hy1b), vd = finish(1, 1, n, p0, p1, lx1, hy1b);
                    s4_f32x4 pv;
#pragma unroll
                    for (int r = 0; r < 4; ++r) pv[r] = (((va[r] + vb[r]) + vc[r]) + vd[r]) * 0.25f;   // order of avgpool2_kernel
                    if ((oy >> 1) < Ho && (ox >> 1) < Wo) store_px(co, (size_t)(oy >> 1) * Wo + (ox >> 1), pv);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        range_commit(a.status, a.range_slot, vmax);
    }
#endif
}

template <int NT, int EPI>
int launch_s41_cfg(const ConvArgs &a0, int B, hipStream_t s) {
    using C = S41Cfg<NT>;
    ConvArgs a = a0;
    a.tilesX = (a.Wout + C::TW - 1) / C::TW;
    a.tilesY = (a.Hout + C::TH - 1) / C::TH;
    size_t lds = C::MAIN;
    a.res_lds_off = -1;
    if (a.res) {
        a.res_rows = res_extent(C::TH, a.res_sh);
        a.res_cols = res_extent(C::TW, a.res_sw);
        const int cs = res_chan_stride(a.res_rows, a.res_cols);
        const size_t need = (size_t)NT * 16 * cs * sizeof(float);
        if (need > 64 * 1024 || (size_t)NT * 16 * cs >= 65536) return fail(PF_EUNSUPPORTED, "conv_s4 1x1: residual window of %zu B does not fit LDS", need);
        a.res_magic_cs = (unsigned)(0x100000000ull / (unsigned)cs) + 1u;          // exact quotients for dividends < 2^16
        a.res_magic_cols = (unsigned)(0x100000000ull / (unsigned)a.res_cols) + 1u;
        a.res_lds_off = C::MAIN / 4;
        lds = C::MAIN + align_up(need, 256);
    }
    static size_t attr_lds = 0;
    if (lds > attr_lds) {
        PF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&conv_s4_1x1_kernel<NT, EPI>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_lds = lds;
    }
    char label[112];
    snprintf(label, sizeof(label), "void pf::conv_s4_1x1_kernel<%d, %d>(pf::ConvArgs)", NT, EPI);
    if (a.res) strncat(label, " +res", sizeof(label) - strlen(label) - 1);
    if (a.pool) strncat(label, " +pool", sizeof(label) - strlen(label) - 1);
    if (a.no_bias) strncat(label, " lowres-half", sizeof(label) - strlen(label) - 1);
    const double px = (double)B * a.Hout * a.Wout;
    ProfScope ps(s, label, 2.0 * px * a.Cout * a.Cin, 4.0 * ((double)B * a.Cin * a.Hin * a.Win + px * a.Cout + (double)a.Cout * a.Cin));
    hipLaunchKernelGGL((conv_s4_1x1_kernel<NT, EPI>), dim3(a.tilesX * a.tilesY, (a.ntiles + NT - 1) / NT, B), dim3(256), lds, s, a);
    PF_LAUNCH_CHECK("conv_s4_1x1_kernel");
    return PF_OK;
}

// the instantiations launch_conv_s4 (conv_s4.hip) dispatches to: EPI = 1 carries the fused epilogue stages
#define PF_S41(NT_) \
    template int launch_s41_cfg<NT_, 0>(const ConvArgs &, int, hipStream_t); \
    template int launch_s41_cfg<NT_, 1>(const ConvArgs &, int, hipStream_t);
PF_S41(1) PF_S41(2) PF_S41(3) PF_S41(4)
#undef PF_S41

}  // namespace pf
