// Semantic confusion matrix on the device: the pixel counts behind IoU / mIoU of the Cityscapes pixel-level
// evaluation (cityscapesscripts.evaluation.evalPixelLevelSemanticLabeling; that package is absent and unpinned: parity unpinned).
// Integers only: no floating-point operation on the device, so two runs of a call give the same bits whatever order the atomics
// arrive in.  Enqueue only.
//
//   conf_count_kernel   grid (pixel chunks, B): a chunk never spans two images.  An image is [head | units | tail]: the head (< 16
//                       pixels) ends where both maps reach the alignment of a lane's load, a unit is what one lane reads per trip - 16
//                       bytes of each map: 16 pixels where both maps are u8, else 4 pixels (4 bytes of a u8 map, 16 of an i32 map,
//                       2 x 16 of an i64 map).  Head and tail go through per element (workgroup 0 of the image, one lane per pixel).
//                       Where no head aligns both maps (u8 at +1 byte against i32 at +4) the map left misaligned is read by element
//                       loads in the same loop: slower, never refused.  A workgroup owns kConfChunkPixels pixels of units; its lanes
//                       load kConfGroup trips at once (the loads do not wait for one another) and fold runs of equal raw
//                       (gt, pred) values in registers - for u8 maps four pixels per compare while a run lasts.  A run that ends is
//                       classified through the 256-entry LUT in LDS (value -> class 0..18, 19 = void) and added to the wave's own
//                       20 x 20 u32 histogram in LDS: one LDS atomic per run, not per pixel.  The fold state is a lane's own and ends
//                       with the workgroup, so nothing carries from image to image.  At the end the wave histograms are summed
//                       and the non-zero counters added to the image's 400 u32 counters in the workspace.
//                       A value outside [0, 256) in an i32 / i64 map (compared in the map's own width) sets the image's flag.
//   conf_finish_kernel  one workgroup: adds the unflagged images' tables into acc and writes per_image, in image order, and ORs the
//                       flags into the sticky status word.
#include "panoptic_ids.h"
#include "pf_common.h"
#include "pf_prof.h"

namespace pf {

constexpr int kConfCls = 20;                  // 19 classes + void
constexpr int kConfCells = kConfCls * kConfCls;
constexpr int kConfVoid = 19;
constexpr int kConfThreads = 256;             // lanes of one count workgroup (the LUT is filled one entry per lane)
constexpr int kConfWaves = kConfThreads / 64;
constexpr int kConfChunkPixels = 16384;       // pixels of units one count workgroup owns, whatever the kinds
constexpr int kConfGroup = 4;                 // trips whose loads are in flight together
enum { kConfU8 = 0, kConfI32 = 1, kConfI64 = 2 };

// workspace: [0, 256) sticky status word; from 256 on everything is zeroed by every call
struct ConfLayout {
    size_t flags, tables, total;
};

static ConfLayout conf_layout(int B) {
    ConfLayout l;
    const size_t b = (size_t)(B > 0 ? B : 1);
    l.flags = 256;
    l.tables = l.flags + align_up(b * sizeof(unsigned), 256);
    l.total = l.tables + align_up(b * kConfCells * sizeof(unsigned), 256);
    return l;
}

struct ConfArgs {
    const void *pred, *gt;
    char *ws;
    ConfLayout l;
    long long *acc, *per_image;
    size_t n_per_image;
    int B, fmt, n_cls;
};

template <int KIND> struct ConfKind;
template <> struct ConfKind<kConfU8> { typedef unsigned char T; };
template <> struct ConfKind<kConfI32> { typedef int T; };
template <> struct ConfKind<kConfI64> { typedef long long T; };

// bytes a lane's load of one unit of P pixels must be aligned to
template <int KIND, int P> __host__ __device__ constexpr int conf_align() { return KIND == kConfU8 ? P : 16; }

struct ConfFold {
    unsigned cur, run, g4, p4;   // cur = gt << 8 | pred; g4 / p4: cur's bytes repeated four times (u8 x u8 path)
};

__device__ __forceinline__ void conf_flush(unsigned *hist, const unsigned char *lut, unsigned key, unsigned n) {
    atomicAdd(hist + lut[key >> 8] * kConfCls + lut[key & 255u], n);
}

__device__ __forceinline__ void conf_pixel(ConfFold &f, unsigned *hist, const unsigned char *lut, unsigned key) {
    if (key == f.cur) {
        ++f.run;
    } else {
        if (f.run) conf_flush(hist, lut, f.cur, f.run);
        f.cur = key;
        f.run = 1;
    }
}

// four u8 pixels of each map in one word: one compare pair while the run lasts
__device__ __forceinline__ void conf_word(ConfFold &f, unsigned *hist, const unsigned char *lut, unsigned gw, unsigned pw) {
    if (gw == f.g4 && pw == f.p4) {
        f.run += 4;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) conf_pixel(f, hist, lut, (((gw >> (8 * k)) & 255u) << 8) | ((pw >> (8 * k)) & 255u));
    f.g4 = (f.cur >> 8) * 0x01010101u;
    f.p4 = (f.cur & 255u) * 0x01010101u;
}

// one element; false: a value outside [0, 256)
template <int KIND>
__device__ __forceinline__ bool conf_load1(const void *base, size_t i, unsigned &v) {
    if (KIND == kConfU8) {
        v = reinterpret_cast<const unsigned char *>(base)[i];
        return true;
    }
    if (KIND == kConfI32) {
        v = (unsigned)reinterpret_cast<const int *>(base)[i];
        return (v >> 8) == 0;
    }
    const unsigned long long x = (unsigned long long)reinterpret_cast<const long long *>(base)[i];
    v = (unsigned)x;
    return (x >> 8) == 0;
}

// four pixels from pixel i on (the generic unit); false: a value outside [0, 256)
template <int KIND>
__device__ __forceinline__ bool conf_load4(const void *base, size_t i, bool aligned, unsigned v[4]) {
    if (!aligned) {
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) ok = conf_load1<KIND>(base, i + k, v[k]) && ok;
        return ok;
    }
    if (KIND == kConfU8) {
        const unsigned w = *reinterpret_cast<const unsigned *>(reinterpret_cast<const unsigned char *>(base) + i);
        v[0] = w & 255u; v[1] = (w >> 8) & 255u; v[2] = (w >> 16) & 255u; v[3] = w >> 24;
        return true;
    }
    if (KIND == kConfI32) {
        const int4 s = *reinterpret_cast<const int4 *>(reinterpret_cast<const int *>(base) + i);
        v[0] = (unsigned)s.x; v[1] = (unsigned)s.y; v[2] = (unsigned)s.z; v[3] = (unsigned)s.w;
        return ((v[0] | v[1] | v[2] | v[3]) >> 8) == 0;
    }
    const longlong2 *s = reinterpret_cast<const longlong2 *>(reinterpret_cast<const long long *>(base) + i);
    const longlong2 s0 = s[0], s1 = s[1];
    v[0] = (unsigned)s0.x; v[1] = (unsigned)s0.y; v[2] = (unsigned)s1.x; v[3] = (unsigned)s1.y;
    return (((unsigned long long)s0.x | (unsigned long long)s0.y | (unsigned long long)s1.x | (unsigned long long)s1.y) >> 8) == 0;
}

// sixteen u8 pixels from pixel i on as four words
__device__ __forceinline__ uint4 conf_load16(const unsigned char *base, size_t i, bool aligned) {
    if (aligned) return *reinterpret_cast<const uint4 *>(base + i);
    unsigned w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        w[k] = (unsigned)base[i + 4 * k] | ((unsigned)base[i + 4 * k + 1] << 8) | ((unsigned)base[i + 4 * k + 2] << 16) |
               ((unsigned)base[i + 4 * k + 3] << 24);
    return uint4{w[0], w[1], w[2], w[3]};
}

template <int PK, int GK>
__global__ __launch_bounds__(kConfThreads) void conf_count_kernel(ConfArgs a) {
    typedef typename ConfKind<PK>::T PT;
    typedef typename ConfKind<GK>::T GT;
    constexpr bool kBytes = PK == kConfU8 && GK == kConfU8;
    constexpr int P = kBytes ? 16 : 4;                          // pixels of one unit
    constexpr int AP = conf_align<PK, P>(), AG = conf_align<GK, P>();
    constexpr size_t kUnitsPerChunk = kConfChunkPixels / P;     // a multiple of kConfGroup * kConfThreads
    static_assert(kUnitsPerChunk % (kConfGroup * kConfThreads) == 0, "a chunk is whole groups of trips");

    __shared__ unsigned hist[kConfWaves][kConfCells];
    __shared__ unsigned char lut[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < kConfWaves * kConfCells; i += kConfThreads) (&hist[0][0])[i] = 0;
    lut[tid] = (unsigned char)((a.fmt == 0 && tid < a.n_cls) ? tid : kConfVoid);
    __syncthreads();
    if (a.fmt == 1 && tid < a.n_cls) lut[kPanTrainId2Id[tid]] = (unsigned char)tid;
    __syncthreads();

    const size_t n = a.n_per_image;
    const PT *pb = reinterpret_cast<const PT *>(a.pred) + (size_t)b * n;
    const GT *gb = reinterpret_cast<const GT *>(a.gt) + (size_t)b * n;
    // the head: the fewest pixels after which both maps are aligned for a lane's load; failing that, the prediction alone
    const uintptr_t pa = (uintptr_t)pb, ga = (uintptr_t)gb;
    size_t head = 16;
    for (int h = 15; h >= 0; --h)
        if ((pa + h * sizeof(PT)) % AP == 0 && (ga + h * sizeof(GT)) % AG == 0) head = h;
    if (head == 16)
        for (int h = 15; h >= 0; --h)
            if ((pa + h * sizeof(PT)) % AP == 0) head = h;
    if (head > n) head = n;
    const bool al_p = (pa + head * sizeof(PT)) % AP == 0, al_g = (ga + head * sizeof(GT)) % AG == 0;
    const size_t units = (n - head) / P, tail0 = head + units * P;   // tail pixels [tail0, n): fewer than P

    unsigned *my = hist[tid >> 6];
    ConfFold f{0u, 0u, 0u, 0u};
    bool ok = true;
    const size_t u0 = (size_t)blockIdx.x * kUnitsPerChunk;
    const size_t u1 = u0 + kUnitsPerChunk < units ? u0 + kUnitsPerChunk : units;
    for (size_t t = u0; t < u1; t += (size_t)kConfGroup * kConfThreads) {
        if constexpr (kBytes) {
            uint4 pv[kConfGroup], gv[kConfGroup];
#pragma unroll
            for (int k = 0; k < kConfGroup; ++k) {
                const size_t u = t + (size_t)k * kConfThreads + tid;
                if (u < u1) {
                    pv[k] = conf_load16(reinterpret_cast<const unsigned char *>(pb), head + u * P, al_p);
                    gv[k] = conf_load16(reinterpret_cast<const unsigned char *>(gb), head + u * P, al_g);
                }
            }
#pragma unroll
            for (int k = 0; k < kConfGroup; ++k) {
                const size_t u = t + (size_t)k * kConfThreads + tid;
                if (u < u1) {
                    conf_word(f, my, lut, gv[k].x, pv[k].x);
                    conf_word(f, my, lut, gv[k].y, pv[k].y);
                    conf_word(f, my, lut, gv[k].z, pv[k].z);
                    conf_word(f, my, lut, gv[k].w, pv[k].w);
                }
            }
        } else {
            unsigned pv[kConfGroup][4], gv[kConfGroup][4];
            bool good[kConfGroup];
#pragma unroll
            for (int k = 0; k < kConfGroup; ++k) {
                const size_t u = t + (size_t)k * kConfThreads + tid;
                good[k] = true;
                if (u < u1) {
                    const bool okp = conf_load4<PK>(pb, head + u * P, al_p, pv[k]);
                    const bool okg = conf_load4<GK>(gb, head + u * P, al_g, gv[k]);
                    good[k] = okp && okg;
                }
            }
#pragma unroll
            for (int k = 0; k < kConfGroup; ++k) {
                const size_t u = t + (size_t)k * kConfThreads + tid;
                if (u >= u1) continue;
                if (!good[k]) {   // the image is flagged below and adds nothing: its pixels need not be counted
                    ok = false;
                    continue;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) conf_pixel(f, my, lut, (gv[k][j] << 8) | pv[k][j]);
            }
        }
    }
    if (f.run) conf_flush(my, lut, f.cur, f.run);
    if (blockIdx.x == 0) {   // head and tail, one lane per pixel: fewer than 16 + P <= 32 of them
        const size_t ntail = n - tail0;
        size_t i = n;
        if ((size_t)tid < head) i = tid;
        else if ((size_t)tid - head < ntail) i = tail0 + ((size_t)tid - head);
        if (i < n) {
            unsigned p, g;
            const bool okp = conf_load1<PK>(pb, i, p), okg = conf_load1<GK>(gb, i, g);
            if (okp && okg) conf_flush(my, lut, (g << 8) | p, 1u);
            else ok = false;
        }
    }
    unsigned *flag = reinterpret_cast<unsigned *>(a.ws + a.l.flags) + b;
    if (!ok) atomicOr(flag, PF_CONF_STATUS_VALUE);
    __syncthreads();
    unsigned *table = reinterpret_cast<unsigned *>(a.ws + a.l.tables) + (size_t)b * kConfCells;
    for (int c = tid; c < kConfCells; c += kConfThreads) {
        unsigned s = 0;
#pragma unroll
        for (int w = 0; w < kConfWaves; ++w) s += hist[w][c];
        if (s) atomicAdd(table + c, s);
    }
}

__global__ __launch_bounds__(512) void conf_finish_kernel(ConfArgs a) {
    const int t = threadIdx.x;
    const unsigned *flags = reinterpret_cast<const unsigned *>(a.ws + a.l.flags);
    const unsigned *tables = reinterpret_cast<const unsigned *>(a.ws + a.l.tables);
    unsigned st = 0;
    long long sum = t < kConfCells ? a.acc[t] : 0;
    for (int b = 0; b < a.B; ++b) {   // image order
        const unsigned f = flags[b];
        st |= f;
        if (t >= kConfCells) continue;
        const long long x = f ? 0 : (long long)tables[(size_t)b * kConfCells + t];
        sum += x;
        if (a.per_image) a.per_image[(size_t)b * kConfCells + t] = x;
    }
    if (t < kConfCells) a.acc[t] = sum;
    if (t == 0 && st) atomicOr(reinterpret_cast<unsigned *>(a.ws), st);
}

template <int PK>
static void conf_launch_gt(int gt_kind, dim3 grid, hipStream_t s, const ConfArgs &a) {
    if (gt_kind == kConfU8) hipLaunchKernelGGL((conf_count_kernel<PK, kConfU8>), grid, dim3(kConfThreads), 0, s, a);
    else if (gt_kind == kConfI32) hipLaunchKernelGGL((conf_count_kernel<PK, kConfI32>), grid, dim3(kConfThreads), 0, s, a);
    else hipLaunchKernelGGL((conf_count_kernel<PK, kConfI64>), grid, dim3(kConfThreads), 0, s, a);
}

}  // namespace pf

extern "C" int pf_confusion_workspace(int B, size_t *bytes) {
    if (!bytes || B < 0) return pf::fail(PF_EINVAL, "pf_confusion_workspace: bad arguments");
    *bytes = pf::conf_layout(B).total;
    return PF_OK;
}

extern "C" int pf_confusion_chunk_pixels(void) { return pf::kConfChunkPixels; }

extern "C" int pf_confusion_accumulate(const void *pred, int pred_kind, const void *gt, int gt_kind, int fmt, int n_cls, int B, int H,
                                       int W, long long *acc, long long *per_image, void *ws, size_t ws_bytes, void *stream) {
    if (B < 0 || H <= 0 || W <= 0 || !acc || !ws || n_cls < 1 || n_cls > pf::kConfVoid || fmt < 0 || fmt > 1 || pred_kind < 0 ||
        pred_kind > 2 || gt_kind < 0 || gt_kind > 2)
        return pf::fail(PF_EINVAL, "pf_confusion_accumulate: bad arguments (B=%d H=%d W=%d n_cls=%d fmt=%d pred_kind=%d gt_kind=%d)", B, H,
                        W, n_cls, fmt, pred_kind, gt_kind);
    if (B == 0) return PF_OK;
    if (!pred || !gt) return pf::fail(PF_EINVAL, "pf_confusion_accumulate: null label map");
    const size_t n = (size_t)H * W;
    if (n >= ((size_t)1 << 32)) return pf::fail(PF_EUNSUPPORTED, "pf_confusion_accumulate: H*W must be below 2^32 (an image's counters are u32)");
    if (B > 65535) return pf::fail(PF_EUNSUPPORTED, "pf_confusion_accumulate: B must be at most 65535");
    const size_t esz[3] = {1, 4, 8};
    if (((uintptr_t)pred % esz[pred_kind]) || ((uintptr_t)gt % esz[gt_kind]))
        return pf::fail(PF_EINVAL, "pf_confusion_accumulate: a label map must be aligned to its element size");
    if (((uintptr_t)ws & 15) || ((uintptr_t)acc & 7) || ((uintptr_t)per_image & 7))
        return pf::fail(PF_EINVAL, "pf_confusion_accumulate: ws must be 16-byte aligned, acc and per_image 8-byte aligned");
    const pf::ConfLayout l = pf::conf_layout(B);
    if (ws_bytes < l.total) return pf::fail(PF_EWORKSPACE, "pf_confusion_accumulate: workspace %zu B < required %zu B", ws_bytes, l.total);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = pf::launch_zero_fill((char *)ws + l.flags, l.total - l.flags, s)) return rc;
    pf::ConfArgs a{pred, gt, (char *)ws, l, acc, per_image, n, B, fmt, n_cls};
    const size_t gx = (n + pf::kConfChunkPixels - 1) / pf::kConfChunkPixels;   // the units are at most n pixels; at least one workgroup
    const dim3 grid((unsigned)gx, (unsigned)B);
    {
        pf::ProfScope ps(s, "pf::conf_count_kernel(pf::ConfArgs)", 0.0, (double)B * n * (double)(esz[pred_kind] + esz[gt_kind]));
        if (pred_kind == pf::kConfU8) pf::conf_launch_gt<pf::kConfU8>(gt_kind, grid, s, a);
        else if (pred_kind == pf::kConfI32) pf::conf_launch_gt<pf::kConfI32>(gt_kind, grid, s, a);
        else pf::conf_launch_gt<pf::kConfI64>(gt_kind, grid, s, a);
        PF_LAUNCH_CHECK("conf_count_kernel");
    }
    hipLaunchKernelGGL(pf::conf_finish_kernel, dim3(1), dim3(512), 0, s, a);
    PF_LAUNCH_CHECK("conf_finish_kernel");
    return PF_OK;
}

extern "C" int pf_confusion_status(const void *ws, void *stream, int *host_status) {
    if (!ws || !host_status) return pf::fail(PF_EINVAL, "pf_confusion_status: null argument");
    unsigned st = 0;
    PF_HIP_CHECK(hipMemcpyAsync(&st, ws, sizeof(unsigned), hipMemcpyDeviceToHost, (hipStream_t)stream));
    PF_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    *host_status = (int)st;
    return PF_OK;
}

extern "C" int pf_confusion_status_reset(void *ws, void *stream) {
    if (!ws) return pf::fail(PF_EINVAL, "pf_confusion_status_reset: null argument");
    return pf::launch_zero_fill(ws, 256, (hipStream_t)stream);
}
