// Semantic confusion matrix on the device: the pixel counts behind IoU / mIoU of the Cityscapes pixel-level
// evaluation (cityscapesscripts.evaluation.evalPixelLevelSemanticLabeling; that package is absent and unpinned: parity unpinned).
// Integers only: no floating-point operation on the device, so two runs of a call give the same bits whatever order the atomics
// arrive in.  Enqueue only.
//
//   conf_count_kernel   the scan of label_scan.h over (pred, gt), both of any kind; 16 pixels per unit where both maps are u8.  Runs of
//                       equal raw (gt, pred) values are folded in registers - for u8 maps four pixels per compare while a run lasts.
//                       A run that ends is classified through the 256-entry LUT in LDS (value -> class 0..18, 19 = void) and added
//                       to the wave's own 20 x 20 u32 histogram in LDS: one LDS atomic per run, not per pixel.  At the end the wave
//                       histograms are summed and the non-zero counters added to the image's 400 u32 counters in the workspace.
//                       A value outside [0, 256) in an i32 / i64 map (compared in the map's own width) sets the image's flag.
//   conf_finish_kernel  one workgroup: adds the unflagged images' tables into acc and writes per_image, in image order, and ORs the
//                       flags into the sticky status word.
#include "label_scan.h"
#include "panoptic_ids.h"
#include "pf_common.h"
#include "pf_prof.h"

namespace pf {

constexpr int kConfCls = 20;                  // 19 classes + void
constexpr int kConfCells = kConfCls * kConfCls;
constexpr int kConfVoid = 19;
constexpr int kConfWaves = kScanThreads / 64;
static_assert(kScanThreads == 256, "the LUT is filled one entry per lane");
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

// the sink of the scan: a wave's histogram; key = gt << 8 | pred
struct ConfFold {
    unsigned *hist;
    const unsigned char *lut;
    unsigned g4, p4;   // the bytes of the fold's current key repeated four times (u8 x u8 path)

    __device__ __forceinline__ void flush(unsigned key, unsigned n) { atomicAdd(hist + lut[key >> 8] * kConfCls + lut[key & 255u], n); }

    // four u8 pixels of each map in one word: one compare pair while the run lasts
    __device__ __forceinline__ void word(RunFold &f, unsigned gw, unsigned pw) {
        if (gw == g4 && pw == p4) {
            f.run += 4;
            return;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) fold_pixel(f, *this, (((gw >> (8 * k)) & 255u) << 8) | ((pw >> (8 * k)) & 255u));
        g4 = (f.cur >> 8) * 0x01010101u;
        p4 = (f.cur & 255u) * 0x01010101u;
    }

    __device__ __forceinline__ void raw(RunFold &f, const uint4 &p, const uint4 (&g)[1]) {
        word(f, g[0].x, p.x);
        word(f, g[0].y, p.y);
        word(f, g[0].z, p.z);
        word(f, g[0].w, p.w);
    }
};

template <int PK, int GK>
__global__ __launch_bounds__(kScanThreads) void conf_count_kernel(ConfArgs a) {
    typedef typename ConfKind<PK>::T PT;
    typedef typename ConfKind<GK>::T GT;
    constexpr int P = (PK == kConfU8 && GK == kConfU8) ? 16 : 4;   // pixels of one unit

    __shared__ unsigned hist[kConfWaves][kConfCells];
    __shared__ unsigned char lut[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < kConfWaves * kConfCells; i += kScanThreads) (&hist[0][0])[i] = 0;
    lut[tid] = (unsigned char)((a.fmt == 0 && tid < a.n_cls) ? tid : kConfVoid);
    __syncthreads();
    if (a.fmt == 1 && tid < a.n_cls) lut[kPanTrainId2Id[tid]] = (unsigned char)tid;
    __syncthreads();

    const size_t n = a.n_per_image;
    const PT *pb = reinterpret_cast<const PT *>(a.pred) + (size_t)b * n;
    const GT *gb = reinterpret_cast<const GT *>(a.gt) + (size_t)b * n;
    ConfFold sink{hist[tid >> 6], lut, 0u, 0u};
    const bool ok = label_scan<PT, GT, 8, P>(pb, gb, n, sink);
    unsigned *flag = reinterpret_cast<unsigned *>(a.ws + a.l.flags) + b;
    if (!ok) atomicOr(flag, PF_CONF_STATUS_VALUE);
    __syncthreads();
    unsigned *table = reinterpret_cast<unsigned *>(a.ws + a.l.tables) + (size_t)b * kConfCells;
    for (int c = tid; c < kConfCells; c += kScanThreads) {
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
    if (gt_kind == kConfU8) hipLaunchKernelGGL((conf_count_kernel<PK, kConfU8>), grid, dim3(kScanThreads), 0, s, a);
    else if (gt_kind == kConfI32) hipLaunchKernelGGL((conf_count_kernel<PK, kConfI32>), grid, dim3(kScanThreads), 0, s, a);
    else hipLaunchKernelGGL((conf_count_kernel<PK, kConfI64>), grid, dim3(kScanThreads), 0, s, a);
}

}  // namespace pf

extern "C" int pf_confusion_workspace(int B, size_t *bytes) {
    if (!bytes || B < 0) return pf::fail(PF_EINVAL, "pf_confusion_workspace: bad arguments");
    *bytes = pf::conf_layout(B).total;
    return PF_OK;
}

extern "C" int pf_confusion_chunk_pixels(void) { return pf::kScanChunkPixels; }

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
    const size_t gx = (n + pf::kScanChunkPixels - 1) / pf::kScanChunkPixels;   // the units are at most n pixels; at least one workgroup
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
    return pf::sticky_status_read("pf_confusion_status", ws, stream, host_status);
}

extern "C" int pf_confusion_status_reset(void *ws, void *stream) { return pf::sticky_status_reset("pf_confusion_status_reset", ws, stream); }
