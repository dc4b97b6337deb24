// Instance-weighted IoU on the device: the per-instance sums behind iIoU of the Cityscapes pixel-level evaluation
// (cityscapesscripts.evaluation.evalPixelLevelSemanticLabeling; that package is absent and unpinned: parity unpinned).  A
// ground-truth instance is a distinct value v > 1000 of an image's instance map (labelId * 1000 + k, always in labelIds); it counts
// when its label's trainId c is a thing class below n_cls.  Enqueue only.
//
//   iiou_count_kernel   integers only.  The scan of label_scan.h over (pred, inst); 16 pixels per unit where the prediction is u8 and
//                       the instance map u16.  A lane folds runs of equal raw (inst, pred) pairs in registers.  A run
//                       that ends is classified once: v <= 1000 leaves at once (stuff, groups, label 1), label = v / 1000 by
//                       multiply-high, thing index through the 128-entry LUT in LDS, k = v - 1000 * label.  It adds (run, run if the
//                       prediction has the instance's class else 0) to the counter pair of slot (thing, k): first in the workgroup's
//                       LDS table (kIiouLdsSlots entries, open addressing, kIiouProbes probes), past that straight to the image's
//                       u32 [8][1000][2] table in the workspace.  The LDS entries are added to that table when the workgroup ends.
//                       Integer adds: the table does not depend on the order the atomics arrive in.
//                       A prediction value outside [0, 256) or an instance value outside [0, 65536) (compared in the map's own
//                       width) sets the image's flag.
//   iiou_weigh_kernel   one workgroup per image, one wave per thing class.  A lane loads its 16 slots (k = step * 64 + lane) at
//                       once; the wave then takes the 1000 slots 64 at a time: each lane computes its slot's w = avg / size,
//                       tp * w and (size - tp) * w (one rounding each), the ballot of the non-zero slots is walked from its
//                       lowest bit and the terms are added in that order - ascending k, which is ascending v within a class.
//                       Writes the image's [8][2] f64 and [8][3] i64 blocks into the workspace.
//   iiou_finish_kernel  one workgroup: adds the unflagged images' blocks (loaded eight images at a time) into acc_inst /
//                       acc_counts in image order, writes the per_image outputs (zero for a flagged image) and ORs the flags
//                       into the sticky status word.
// Built with FP contraction off; the f64 operations are the _rn intrinsics besides.
#include "label_scan.h"
#include "panoptic_ids.h"
#include "pf_common.h"
#include "pf_prof.h"

namespace pf {

constexpr int kIiouThings = 8;                  // trainIds 11..18
constexpr int kIiouIndices = 1000;              // k of labelId * 1000 + k
constexpr int kIiouSlots = kIiouThings * kIiouIndices;
constexpr int kIiouLdsBits = 9;
constexpr int kIiouLdsSlots = 1 << kIiouLdsBits;   // entries of a workgroup's LDS table
constexpr int kIiouProbes = 4;
constexpr unsigned kIiouEmpty = 0xffffffffu;
constexpr unsigned kIiouDiv1000 = 4294968u;     // ceil(2^32 / 1000): __umulhi(v, .) == v / 1000 for v < 65536 (checked below)
constexpr int kIiouNoThing = 255;
enum { kIiouPredU8 = 0, kIiouPredI32 = 1, kIiouPredI64 = 2 };
enum { kIiouInstU16 = 0, kIiouInstI32 = 1, kIiouInstI64 = 2 };

constexpr unsigned iiou_div1000(unsigned v) { return (unsigned)(((unsigned long long)v * kIiouDiv1000) >> 32); }
constexpr bool iiou_div_is_exact() {   // the product is monotonic in v: the first and last value of every thousand decide
    for (unsigned q = 0; q < 66u; ++q)
        if (iiou_div1000(q * 1000u) != q || iiou_div1000(q * 1000u + 999u) != q) return false;
    return true;
}
static_assert(iiou_div_is_exact(), "the multiplier divides every u16 value by 1000");

// the evaluator's average instance size per thing class, as remembered (semantic_iou.AVG_CLASS_SIZE is the host's copy)
__device__ const double kIiouAvgSize[kIiouThings] = {3462.4756337644, 3930.4788056518, 12794.0202738185, 27855.1264367816,
                                                     35732.1511111111, 67422.8757396450, 6298.7200839748, 4672.3249222261};

// workspace: [0, 256) sticky status word; from 256 on everything is zeroed by every call
struct IiouLayout {
    size_t flags, sums, counts, tables, total;
};

static IiouLayout iiou_layout(int B) {
    IiouLayout l;
    const size_t b = (size_t)(B > 0 ? B : 1);
    l.flags = 256;
    l.sums = l.flags + align_up(b * sizeof(unsigned), 256);
    l.counts = l.sums + align_up(b * kIiouThings * 2 * sizeof(double), 256);
    l.tables = l.counts + align_up(b * kIiouThings * 3 * sizeof(long long), 256);
    l.total = l.tables + align_up(b * kIiouSlots * 2 * sizeof(unsigned), 256);
    return l;
}

struct IiouArgs {
    const void *pred, *inst;
    char *ws;
    IiouLayout l;
    double *acc_inst, *per_image;
    long long *acc_counts, *per_image_counts;
    size_t n_per_image;
    int B, fmt, n_cls;
};

template <int KIND> struct IiouPred;
template <> struct IiouPred<kIiouPredU8> { typedef unsigned char T; };
template <> struct IiouPred<kIiouPredI32> { typedef int T; };
template <> struct IiouPred<kIiouPredI64> { typedef long long T; };
template <int KIND> struct IiouInst;
template <> struct IiouInst<kIiouInstU16> { typedef unsigned short T; };
template <> struct IiouInst<kIiouInstI32> { typedef int T; };
template <> struct IiouInst<kIiouInstI64> { typedef long long T; };

// a workgroup's table in LDS and the image's table in the workspace
struct IiouTables {
    unsigned *key;              // [kIiouLdsSlots] slot or kIiouEmpty
    unsigned *cnt;              // [kIiouLdsSlots][2]
    unsigned *image;            // [kIiouSlots][2]
    const unsigned char *lut;   // label -> thing index 0..7 or kIiouNoThing
    int fmt;
};

__device__ __forceinline__ void iiou_add(const IiouTables &t, unsigned slot, unsigned n, unsigned tp) {
    unsigned h = (slot * 0x9E3779B1u) >> (32 - kIiouLdsBits);
#pragma unroll 1
    for (int probe = 0; probe < kIiouProbes; ++probe) {
        const unsigned old = atomicCAS(t.key + h, kIiouEmpty, slot);
        if (old == kIiouEmpty || old == slot) {
            atomicAdd(t.cnt + 2 * h, n);
            if (tp) atomicAdd(t.cnt + 2 * h + 1, tp);
            return;
        }
        h = (h + 1) & (kIiouLdsSlots - 1);
    }
    atomicAdd(t.image + 2 * slot, n);
    if (tp) atomicAdd(t.image + 2 * slot + 1, tp);
}

// a finished run of n pixels of key = inst << 8 | pred
__device__ __forceinline__ void iiou_flush(const IiouTables &t, unsigned key, unsigned n) {
    const unsigned v = key >> 8, p = key & 255u;
    if (v <= 1000u) return;
    const unsigned label = __umulhi(v, kIiouDiv1000);   // at most 65
    const unsigned thing = t.lut[label];
    if (thing == kIiouNoThing) return;
    const unsigned want = t.fmt ? label : thing + kPanFirstThing;
    iiou_add(t, thing * kIiouIndices + (v - label * 1000u), n, p == want ? n : 0u);
}

// the sink of the scan; key = inst << 8 | pred
struct IiouFold {
    IiouTables t;
    unsigned p4, i2;   // the prediction byte / instance half of the fold's current key repeated (u8 x u16 path)

    __device__ __forceinline__ void flush(unsigned key, unsigned n) { iiou_flush(t, key, n); }

    // four pixels: a word of prediction bytes and two words of instance halves; one compare triple while the run lasts
    __device__ __forceinline__ void word(RunFold &f, unsigned pw, unsigned i0, unsigned i1) {
        if (pw == p4 && i0 == i2 && i1 == i2) {
            f.run += 4;
            return;
        }
        fold_pixel(f, *this, ((i0 & 65535u) << 8) | (pw & 255u));
        fold_pixel(f, *this, ((i0 >> 16) << 8) | ((pw >> 8) & 255u));
        fold_pixel(f, *this, ((i1 & 65535u) << 8) | ((pw >> 16) & 255u));
        fold_pixel(f, *this, ((i1 >> 16) << 8) | (pw >> 24));
        p4 = (f.cur & 255u) * 0x01010101u;
        i2 = (f.cur >> 8) * 0x00010001u;
    }

    __device__ __forceinline__ void raw(RunFold &f, const uint4 &p, const uint4 (&i)[2]) {
        word(f, p.x, i[0].x, i[0].y);
        word(f, p.y, i[0].z, i[0].w);
        word(f, p.z, i[1].x, i[1].y);
        word(f, p.w, i[1].z, i[1].w);
    }
};

template <int PK, int IK>
__global__ __launch_bounds__(kScanThreads) void iiou_count_kernel(IiouArgs a) {
    typedef typename IiouPred<PK>::T PT;
    typedef typename IiouInst<IK>::T IT;
    constexpr int P = (PK == kIiouPredU8 && IK == kIiouInstU16) ? 16 : 4;   // pixels of one unit

    __shared__ unsigned key[kIiouLdsSlots];
    __shared__ unsigned cnt[kIiouLdsSlots][2];
    __shared__ unsigned char lut[128];
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < kIiouLdsSlots; i += kScanThreads) {
        key[i] = kIiouEmpty;
        cnt[i][0] = 0;
        cnt[i][1] = 0;
    }
    if (tid < 128) lut[tid] = (unsigned char)kIiouNoThing;
    __syncthreads();
    if (tid >= kPanFirstThing && tid < a.n_cls) lut[kPanTrainId2Id[tid]] = (unsigned char)(tid - kPanFirstThing);
    __syncthreads();

    const size_t n = a.n_per_image;
    const PT *pb = reinterpret_cast<const PT *>(a.pred) + (size_t)b * n;
    const IT *ib = reinterpret_cast<const IT *>(a.inst) + (size_t)b * n;
    IiouFold sink{{key, &cnt[0][0], reinterpret_cast<unsigned *>(a.ws + a.l.tables) + (size_t)b * kIiouSlots * 2, lut, a.fmt}, 0u, 0u};
    const IiouTables &t = sink.t;
    const bool ok = label_scan<PT, IT, 16, P>(pb, ib, n, sink);
    if (!ok) atomicOr(reinterpret_cast<unsigned *>(a.ws + a.l.flags) + b, PF_IIOU_STATUS_VALUE);
    __syncthreads();
    for (int i = tid; i < kIiouLdsSlots; i += kScanThreads) {
        const unsigned slot = key[i];
        if (slot == kIiouEmpty) continue;
        atomicAdd(t.image + 2 * slot, cnt[i][0]);
        if (cnt[i][1]) atomicAdd(t.image + 2 * slot + 1, cnt[i][1]);
    }
}

__global__ __launch_bounds__(kIiouThings * 64) void iiou_weigh_kernel(IiouArgs a) {
    const int b = blockIdx.x, thing = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint2 *slots = reinterpret_cast<const uint2 *>(a.ws + a.l.tables) + ((size_t)b * kIiouThings + thing) * kIiouIndices;
    const double avg = kIiouAvgSize[thing];
    double itp = 0.0, ifn = 0.0;
    long long instances = 0, pixels = 0, hits = 0;
    constexpr int kSteps = (kIiouIndices + 63) / 64;
    uint2 xs[kSteps];   // (size, tp) of slot step * 64 + lane: every load issued before the first is used
#pragma unroll
    for (int step = 0; step < kSteps; ++step) {
        const int k = step * 64 + lane;
        xs[step] = k < kIiouIndices ? slots[k] : uint2{0u, 0u};
    }
#pragma unroll
    for (int step = 0; step < kSteps; ++step) {
        const uint2 x = xs[step];
        double tpw = 0.0, fnw = 0.0;
        if (x.x) {
            const double w = __ddiv_rn(avg, (double)x.x);
            tpw = __dmul_rn((double)x.y, w);
            fnw = __dmul_rn((double)(x.x - x.y), w);
        }
        pixels += x.x;
        hits += x.y;
        unsigned long long m = __ballot(x.x != 0u);
        instances += __popcll(m);
        while (m) {   // ascending k: the same walk in every lane
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            itp = __dadd_rn(itp, __shfl(tpw, l));
            ifn = __dadd_rn(ifn, __shfl(fnw, l));
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        pixels += __shfl_down(pixels, d);
        hits += __shfl_down(hits, d);
    }
    if (lane == 0) {
        double *sums = reinterpret_cast<double *>(a.ws + a.l.sums) + ((size_t)b * kIiouThings + thing) * 2;
        long long *counts = reinterpret_cast<long long *>(a.ws + a.l.counts) + ((size_t)b * kIiouThings + thing) * 3;
        sums[0] = itp;
        sums[1] = ifn;
        counts[0] = instances;
        counts[1] = pixels;
        counts[2] = hits;
    }
}

__global__ __launch_bounds__(64) void iiou_finish_kernel(IiouArgs a) {
    constexpr int NS = kIiouThings * 2, NC = kIiouThings * 3;
    const int t = threadIdx.x;
    const unsigned *flags = reinterpret_cast<const unsigned *>(a.ws + a.l.flags);
    const double *sums = reinterpret_cast<const double *>(a.ws + a.l.sums);
    const long long *counts = reinterpret_cast<const long long *>(a.ws + a.l.counts);
    unsigned st = 0;
    double s = t < NS ? a.acc_inst[t] : 0.0;
    long long c = (t >= NS && t < NS + NC) ? a.acc_counts[t - NS] : 0;
    constexpr int G = 8;   // images whose blocks are loaded together: the loads do not wait for the stores between them
    for (int b0 = 0; b0 < a.B; b0 += G) {   // image order
        unsigned f[G];
        double xs[G];
        long long xc[G];
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int b = b0 + j;
            f[j] = b < a.B ? flags[b] : 0u;
            xs[j] = (b < a.B && t < NS) ? sums[(size_t)b * NS + t] : 0.0;
            xc[j] = (b < a.B && t >= NS && t < NS + NC) ? counts[(size_t)b * NC + (t - NS)] : 0;
        }
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int b = b0 + j;
            if (b >= a.B) break;
            st |= f[j];
            if (t < NS) {
                const double x = f[j] ? 0.0 : xs[j];
                s = __dadd_rn(s, x);
                if (a.per_image) a.per_image[(size_t)b * NS + t] = x;
            } else if (t < NS + NC) {
                const long long x = f[j] ? 0 : xc[j];
                c += x;
                if (a.per_image_counts) a.per_image_counts[(size_t)b * NC + (t - NS)] = x;
            }
        }
    }
    if (t < NS) a.acc_inst[t] = s;
    else if (t < NS + NC) a.acc_counts[t - NS] = c;
    if (t == 0 && st) atomicOr(reinterpret_cast<unsigned *>(a.ws), st);
}

template <int PK>
static void iiou_launch_inst(int inst_kind, dim3 grid, hipStream_t s, const IiouArgs &a) {
    if (inst_kind == kIiouInstU16) hipLaunchKernelGGL((iiou_count_kernel<PK, kIiouInstU16>), grid, dim3(kScanThreads), 0, s, a);
    else if (inst_kind == kIiouInstI32) hipLaunchKernelGGL((iiou_count_kernel<PK, kIiouInstI32>), grid, dim3(kScanThreads), 0, s, a);
    else hipLaunchKernelGGL((iiou_count_kernel<PK, kIiouInstI64>), grid, dim3(kScanThreads), 0, s, a);
}

}  // namespace pf

extern "C" int pf_iiou_workspace(int B, size_t *bytes) {
    if (!bytes || B < 0) return pf::fail(PF_EINVAL, "pf_iiou_workspace: bad arguments");
    *bytes = pf::iiou_layout(B).total;
    return PF_OK;
}

extern "C" int pf_iiou_chunk_pixels(void) { return pf::kScanChunkPixels; }

extern "C" int pf_iiou_accumulate(const void *pred, int pred_kind, const void *inst, int inst_kind, int fmt, int n_cls, int B, int H,
                                  int W, double *acc_inst, long long *acc_counts, double *per_image, long long *per_image_counts,
                                  void *ws, size_t ws_bytes, void *stream) {
    if (B < 0 || H <= 0 || W <= 0 || !acc_inst || !acc_counts || !ws || n_cls < 1 || n_cls > 19 || fmt < 0 || fmt > 1 || pred_kind < 0 ||
        pred_kind > 2 || inst_kind < 0 || inst_kind > 2)
        return pf::fail(PF_EINVAL, "pf_iiou_accumulate: bad arguments (B=%d H=%d W=%d n_cls=%d fmt=%d pred_kind=%d inst_kind=%d)", B, H, W,
                        n_cls, fmt, pred_kind, inst_kind);
    if (B == 0) return PF_OK;
    if (!pred || !inst) return pf::fail(PF_EINVAL, "pf_iiou_accumulate: null map");
    const size_t n = (size_t)H * W;
    if (n >= ((size_t)1 << 32)) return pf::fail(PF_EUNSUPPORTED, "pf_iiou_accumulate: H*W must be below 2^32 (an instance's counters are u32)");
    if (B > 65535) return pf::fail(PF_EUNSUPPORTED, "pf_iiou_accumulate: B must be at most 65535");
    const size_t psz[3] = {1, 4, 8}, isz[3] = {2, 4, 8};
    if (((uintptr_t)pred % psz[pred_kind]) || ((uintptr_t)inst % isz[inst_kind]))
        return pf::fail(PF_EINVAL, "pf_iiou_accumulate: a map must be aligned to its element size");
    if (((uintptr_t)ws & 15) || ((uintptr_t)acc_inst & 7) || ((uintptr_t)acc_counts & 7) || ((uintptr_t)per_image & 7) ||
        ((uintptr_t)per_image_counts & 7))
        return pf::fail(PF_EINVAL, "pf_iiou_accumulate: ws must be 16-byte aligned, the accumulators and per-image outputs 8-byte aligned");
    const pf::IiouLayout l = pf::iiou_layout(B);
    if (ws_bytes < l.total) return pf::fail(PF_EWORKSPACE, "pf_iiou_accumulate: workspace %zu B < required %zu B", ws_bytes, l.total);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = pf::launch_zero_fill((char *)ws + l.flags, l.total - l.flags, s)) return rc;
    pf::IiouArgs a{pred, inst, (char *)ws, l, acc_inst, per_image, acc_counts, per_image_counts, n, B, fmt, n_cls};
    const size_t gx = (n + pf::kScanChunkPixels - 1) / pf::kScanChunkPixels;   // the units are at most n pixels; at least one workgroup
    const dim3 grid((unsigned)gx, (unsigned)B);
    {
        pf::ProfScope ps(s, "pf::iiou_count_kernel(pf::IiouArgs)", 0.0, (double)B * n * (double)(psz[pred_kind] + isz[inst_kind]));
        if (pred_kind == pf::kIiouPredU8) pf::iiou_launch_inst<pf::kIiouPredU8>(inst_kind, grid, s, a);
        else if (pred_kind == pf::kIiouPredI32) pf::iiou_launch_inst<pf::kIiouPredI32>(inst_kind, grid, s, a);
        else pf::iiou_launch_inst<pf::kIiouPredI64>(inst_kind, grid, s, a);
        PF_LAUNCH_CHECK("iiou_count_kernel");
    }
    {
        pf::ProfScope ps(s, "pf::iiou_weigh_kernel(pf::IiouArgs)", 0.0, (double)B * pf::kIiouSlots * 8.0);
        hipLaunchKernelGGL(pf::iiou_weigh_kernel, dim3((unsigned)B), dim3(pf::kIiouThings * 64), 0, s, a);
        PF_LAUNCH_CHECK("iiou_weigh_kernel");
    }
    {
        pf::ProfScope ps(s, "pf::iiou_finish_kernel(pf::IiouArgs)", 0.0, (double)B * pf::kIiouThings * 40.0);
        hipLaunchKernelGGL(pf::iiou_finish_kernel, dim3(1), dim3(64), 0, s, a);
        PF_LAUNCH_CHECK("iiou_finish_kernel");
    }
    return PF_OK;
}

extern "C" int pf_iiou_status(const void *ws, void *stream, int *host_status) {
    return pf::sticky_status_read("pf_iiou_status", ws, stream, host_status);
}

extern "C" int pf_iiou_status_reset(void *ws, void *stream) { return pf::sticky_status_reset("pf_iiou_status_reset", ws, stream); }
