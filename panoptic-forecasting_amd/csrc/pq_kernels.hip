// Panoptic quality on the device: the segment matching of the standard panoptic evaluation, the last
// stage of scripts/fg/run_fg_eval_panoptic.sh (python -m cityscapesscripts.evaluation.evalPanopticSemanticLabeling; that package
// is absent and unpinned: layout and parity unpinned).  Integer-exact counts, one fp64 division per candidate match, enqueue only.
//
//   pq_count_kernel   grid (pixel chunks, B).  Every lane reads 16 bytes (i32) or 2 x 16 bytes (i64) of each map per trip = 4 pixels,
//                     folds runs of equal (gt, pred) pairs in its registers (label maps are runs; the fold carries over from trip to
//                     trip), and adds (key = gt << 16 | pred, run length) to a workgroup-private open-addressing table in LDS:
//                     kPqLdsSlots slots of one u64 = key u32 : count u32.  A slot is empty iff the whole word is 0 (a live slot counts
//                     >= 1 pixel), so the key takes one 64-bit integer compare-and-swap and the count one integer add.  The LDS
//                     table is flushed once per workgroup into the image's table in the workspace (kPqSlots slots, same form).
//                     A key that finds no room in LDS (more than kPqLdsSlots / 2 keys claimed, or every probe taken) goes straight
//                     to the image's table: nothing is lost or counted twice.  A value outside [0, 65536) (compared in the map's own
//                     width) or an image table with no room sets the image's flag; every probe sequence is bounded by the table size.
//   pq_match_kernel   one workgroup per image.  A: walks the pair table and forms g_area[g], p_area[p] (segment tables of kPqSlots
//                     slots in the workspace, id u32 : area u32, void folded into one pseudo-segment), p_void[p] and p_crowd[p].
//                     B: for every pair of equal category whose gt segment is neither void nor crowd,
//                     iou = inter / (g_area + p_area - inter - p_void[p]) in fp64; iou > 0.5 marks both segments and stores the iou at
//                     [class][0 for a value < 1000, else 1 + value % 1000]: a table in ascending gt id.  C: TP / FN over the gt
//                     segments, FP over the unmatched predictions unless 2 (p_void + p_crowd) > p_area.  D: one wave per class adds
//                     that class's ious in table order, i.e. ascending gt id, whatever order the atomics arrived in.
//   pq_finish_kernel  adds the B rows into the caller's accumulators in image order (flagged images add nothing) and ORs the flags
//                     into the sticky status word.
// Floating point is only the division and the ordered sums: two runs of a call give the same bits.
#include <type_traits>

#include "label_scan.h"
#include "panoptic_ids.h"
#include "pf_common.h"
#include "pf_prof.h"

namespace pf {

constexpr int kPqSlots = 8192;          // distinct (gt, pred) pairs an image may hold (a Cityscapes image has a few hundred)
constexpr int kPqLdsSlots = 1024;       // per workgroup; at most half are claimed before new keys go to the image's table
constexpr int kPqMaxCls = 19;
constexpr int kPqIdsPerClass = 1001;    // value c (stuff form) and c * 1000 + 0..999
constexpr unsigned kPqVoid = 0x10000u;  // pseudo-segment id of everything void (no 16-bit value)
constexpr int kPqCountThreads = 256;    // lanes of one count workgroup
// lds_add reads `used` before it claims and counts after: every lane of the workgroup may pass the check at kPqLdsSlots / 2 - 1 together,
// so up to kPqLdsSlots / 2 + kPqCountThreads slots get claimed.  That must stay below the table size, or a probe walk finds no empty slot.
static_assert(kPqLdsSlots / 2 + kPqCountThreads < kPqLdsSlots, "the LDS pair table could fill: raise kPqLdsSlots or lower the claim cap");
constexpr int kPqTripsPerGroup = 8;     // least work of one count workgroup: 8 trips x 256 lanes x 4 pixels

typedef unsigned long long u64;

// workspace: [0, 256) sticky status word; from 256 on everything is zeroed by every call
struct PqLayout {
    size_t flags, rows, images, image_stride, total;
    size_t pairs, gseg, pseg, pvoid, pcrowd, pmatched, iou;   // inside one image's block
};

static PqLayout pq_layout(int B) {
    PqLayout l;
    const size_t b = (size_t)(B > 0 ? B : 1);
    l.flags = 256;
    l.rows = l.flags + align_up(b * sizeof(unsigned), 256);
    l.images = l.rows + align_up(b * kPqMaxCls * 4 * sizeof(double), 256);
    size_t o = 0;
    l.pairs = o; o += (size_t)kPqSlots * 8;
    l.gseg = o; o += (size_t)kPqSlots * 8;
    l.pseg = o; o += (size_t)kPqSlots * 8;
    l.pvoid = o; o += (size_t)kPqSlots * 4;
    l.pcrowd = o; o += (size_t)kPqSlots * 4;
    l.pmatched = o; o += (size_t)kPqSlots * 4;
    l.iou = o; o += align_up((size_t)kPqMaxCls * kPqIdsPerClass * 8, 256);
    l.image_stride = o;
    l.total = l.images + b * l.image_stride;
    return l;
}

struct PqArgs {
    const void *pred, *gt;
    char *ws;
    PqLayout l;
    double *acc, *per_image;
    size_t n_per_image;
    int B, fmt, crowd, n_cls;
};

__device__ __forceinline__ u64 ld64(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned ld32(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <int LOG2>
__device__ __forceinline__ unsigned pq_hash(unsigned key) { return (key * 0x9E3779B1u) >> (32 - LOG2); }

// adds n to key's slot of an image-level table (claiming one if need be); the slot, or -1 when all kPqSlots probes are taken
__device__ __forceinline__ int table_add(u64 *tab, unsigned key, unsigned n) {
    unsigned h = pq_hash<13>(key);
    for (int probe = 0; probe < kPqSlots; ++probe, h = (h + 1) & (kPqSlots - 1)) {
        u64 v = ld64(tab + h);
        if (v == 0) {
            v = atomicCAS(tab + h, 0ull, ((u64)key << 32) | n);
            if (v == 0) return (int)h;
        }
        if ((unsigned)(v >> 32) == key) {
            atomicAdd(tab + h, (u64)n);
            return (int)h;
        }
    }
    return -1;
}

__device__ __forceinline__ int table_find(const u64 *tab, unsigned key) {
    unsigned h = pq_hash<13>(key);
    for (int probe = 0; probe < kPqSlots; ++probe, h = (h + 1) & (kPqSlots - 1)) {
        const u64 v = ld64(tab + h);
        if (v == 0) return -1;
        if ((unsigned)(v >> 32) == key) return (int)h;
    }
    return -1;
}

__device__ __forceinline__ void image_add(u64 *pairs, unsigned *flag, unsigned key, unsigned n) {
    if (ld32(flag) & PF_PQ_STATUS_FULL) return;   // the image is lost already: no more full-length probe walks
    if (table_add(pairs, key, n) < 0) atomicOr(flag, PF_PQ_STATUS_FULL);
}

__device__ __forceinline__ void lds_add(u64 *tab, unsigned *used, u64 *pairs, unsigned *flag, unsigned key, unsigned n) {
    unsigned h = pq_hash<10>(key);
    for (int probe = 0; probe < kPqLdsSlots; ++probe, h = (h + 1) & (kPqLdsSlots - 1)) {
        u64 v = *(volatile u64 *)(tab + h);
        if (v == 0) {
            // Soft cap: keeps LDS probe walks short, new keys go to the image's table.  The read is not atomic with the claim below,
            // so the lanes in flight can overshoot it by one each; the static_assert at kPqCountThreads keeps the table from filling.
            if (*(volatile unsigned *)used >= kPqLdsSlots / 2) break;
            v = atomicCAS(tab + h, 0ull, ((u64)key << 32) | n);
            if (v == 0) {
                atomicAdd(used, 1u);
                return;
            }
        }
        if ((unsigned)(v >> 32) == key) {
            atomicAdd(tab + h, (u64)n);
            return;
        }
    }
    image_add(pairs, flag, key, n);
}

template <bool P64, bool G64>
__global__ __launch_bounds__(kPqCountThreads) void pq_count_kernel(PqArgs a) {
    typedef typename std::conditional<P64, long long, int>::type PT;
    typedef typename std::conditional<G64, long long, int>::type GT;
    __shared__ u64 tab[kPqLdsSlots];
    __shared__ unsigned used;
    const int b = blockIdx.y;
    for (int s = threadIdx.x; s < kPqLdsSlots; s += kPqCountThreads) tab[s] = 0;
    if (threadIdx.x == 0) used = 0;
    __syncthreads();
    char *img = a.ws + a.l.images + (size_t)b * a.l.image_stride;
    u64 *pairs = reinterpret_cast<u64 *>(img + a.l.pairs);
    unsigned *flag = reinterpret_cast<unsigned *>(a.ws + a.l.flags) + b;
    const PT *pb = reinterpret_cast<const PT *>(a.pred) + (size_t)b * a.n_per_image;
    const GT *gb = reinterpret_cast<const GT *>(a.gt) + (size_t)b * a.n_per_image;

    const size_t n4 = a.n_per_image >> 2;
    const size_t trips = (n4 + kPqCountThreads - 1) / kPqCountThreads, per = (trips + gridDim.x - 1) / gridDim.x;
    const size_t t0 = (size_t)blockIdx.x * per, t1 = t0 + per < trips ? t0 + per : trips;
    unsigned cur = 0, run = 0;
    bool ok = true;
    for (size_t t = t0; t < t1; ++t) {
        const size_t q = t * kPqCountThreads + threadIdx.x;
        if (q >= n4) break;
        unsigned p[4], g[4];
        const bool okp = load4<PT, 16>(pb, 4 * q, true, p), okg = load4<GT, 16>(gb, 4 * q, true, g);   // false: a value outside [0, 65536)
        if (!(okp && okg)) {   // the image is flagged below and adds nothing: its pairs need not be counted
            ok = false;
            continue;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned key = (g[k] << 16) | p[k];
            if (key == cur) {
                ++run;
            } else {
                if (run) lds_add(tab, &used, pairs, flag, cur, run);
                cur = key;
                run = 1;
            }
        }
    }
    if (run) lds_add(tab, &used, pairs, flag, cur, run);
    if (!ok) atomicOr(flag, PF_PQ_STATUS_VALUE);
    __syncthreads();
    for (int s = threadIdx.x; s < kPqLdsSlots; s += kPqCountThreads) {
        const u64 v = tab[s];
        if (v) image_add(pairs, flag, (unsigned)(v >> 32), (unsigned)v);
    }
}

// trainId of a value's category, or -1 when it is none of the n_cls evaluated classes (void)
__device__ __forceinline__ int pq_category(unsigned v, int fmt, int n_cls, const int *inv) {
    if (v >= kPqVoid) return -1;
    const int base = v >= 1000 ? (int)(v / 1000) : (int)v;
    int t = base;
    if (fmt) t = base < kPanMaxId ? inv[base] : -1;
    return (t >= 0 && t < n_cls) ? t : -1;
}

__device__ __forceinline__ bool pq_is_crowd(unsigned v, int cat, int crowd) { return crowd && v < 1000 && cat >= kPanFirstThing; }
__device__ __forceinline__ int pq_id_slot(unsigned v) { return v < 1000 ? 0 : 1 + (int)(v % 1000); }

__global__ __launch_bounds__(1024) void pq_match_kernel(PqArgs a) {
    __shared__ int inv[kPanMaxId];
    __shared__ unsigned cnt[kPqMaxCls * 3];   // TP, FP, FN
    const int b = blockIdx.x, tid = threadIdx.x;
    if (reinterpret_cast<const unsigned *>(a.ws + a.l.flags)[b]) return;   // flagged by the count pass: its row stays zero
    if (tid < kPanMaxId) inv[tid] = -1;
    if (tid < kPqMaxCls * 3) cnt[tid] = 0;
    __syncthreads();
    if (tid < kPqMaxCls) inv[kPanTrainId2Id[tid]] = tid;
    __syncthreads();
    char *img = a.ws + a.l.images + (size_t)b * a.l.image_stride;
    const u64 *pairs = reinterpret_cast<const u64 *>(img + a.l.pairs);
    u64 *gseg = reinterpret_cast<u64 *>(img + a.l.gseg), *pseg = reinterpret_cast<u64 *>(img + a.l.pseg);
    unsigned *pvoid = reinterpret_cast<unsigned *>(img + a.l.pvoid), *pcrowd = reinterpret_cast<unsigned *>(img + a.l.pcrowd);
    unsigned *pmatched = reinterpret_cast<unsigned *>(img + a.l.pmatched);
    u64 *iou_tab = reinterpret_cast<u64 *>(img + a.l.iou);   // fp64 bit patterns, [class][kPqIdsPerClass]

    // every thread owns kPer slots of each table; it loads them at once (the loads do not wait for one another)
    constexpr int kPer = kPqSlots / 1024;
    u64 pr[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) pr[i] = pairs[tid + i * 1024];
    // A: areas.  Distinct segments <= distinct pairs <= kPqSlots, so the segment tables always have room.
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const u64 v = pr[i];
        if (!v) continue;
        const unsigned key = (unsigned)(v >> 32), n = (unsigned)v, g = key >> 16, p = key & 0xffffu;
        const int gc = pq_category(g, a.fmt, a.n_cls, inv), pc = pq_category(p, a.fmt, a.n_cls, inv);
        table_add(gseg, gc < 0 ? kPqVoid : g, n);
        const int ps = table_add(pseg, pc < 0 ? kPqVoid : p, n);
        if (ps < 0) continue;
        if (gc < 0) atomicAdd(pvoid + ps, n);
        else if (pq_is_crowd(g, gc, a.crowd) && gc == pc) atomicAdd(pcrowd + ps, n);
    }
    __threadfence();
    __syncthreads();
    // B: matches
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const u64 v = pr[i];
        if (!v) continue;
        const unsigned key = (unsigned)(v >> 32), n = (unsigned)v, g = key >> 16, p = key & 0xffffu;
        const int gc = pq_category(g, a.fmt, a.n_cls, inv), pc = pq_category(p, a.fmt, a.n_cls, inv);
        if (gc < 0 || gc != pc || pq_is_crowd(g, gc, a.crowd)) continue;
        const int gs = table_find(gseg, g), ps = table_find(pseg, p);
        if (gs < 0 || ps < 0) continue;
        const long long ga = (unsigned)ld64(gseg + gs), pa = (unsigned)ld64(pseg + ps), pv = ld32(pvoid + ps);
        const double iou = (double)n / (double)(ga + pa - (long long)n - pv);
        if (iou > 0.5) {   // unique per segment: two disjoint parts cannot both exceed half
            __hip_atomic_store(iou_tab + gc * kPqIdsPerClass + pq_id_slot(g), (u64)__double_as_longlong(iou), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(pmatched + ps, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __threadfence();
    __syncthreads();
    // C: counts
    u64 gv[kPer], pw[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        gv[i] = ld64(gseg + tid + i * 1024);
        pw[i] = ld64(pseg + tid + i * 1024);
    }
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int s = tid + i * 1024;
        const u64 v = gv[i];
        if (v) {
            const unsigned g = (unsigned)(v >> 32);
            const int gc = pq_category(g, a.fmt, a.n_cls, inv);
            if (gc >= 0 && !pq_is_crowd(g, gc, a.crowd))
                atomicAdd(cnt + gc * 3 + (ld64(iou_tab + gc * kPqIdsPerClass + pq_id_slot(g)) ? 0 : 2), 1u);
        }
        const u64 w = pw[i];
        if (w) {
            const unsigned p = (unsigned)(w >> 32);
            const int pc = pq_category(p, a.fmt, a.n_cls, inv);
            if (pc >= 0 && !ld32(pmatched + s)) {
                const u64 excused = (u64)ld32(pvoid + s) + ld32(pcrowd + s);
                if (!(2 * excused > (u64)(unsigned)w)) atomicAdd(cnt + pc * 3 + 1, 1u);
            }
        }
    }
    __syncthreads();
    // D: one wave per class adds its ious in ascending gt id (every lane carries the same sum)
    double *row = reinterpret_cast<double *>(a.ws + a.l.rows) + (size_t)b * kPqMaxCls * 4;
    const int wave = tid >> 6, lane = tid & 63;
    for (int c = wave; c < a.n_cls; c += 16) {
        constexpr int kChunks = (kPqIdsPerClass + 63) / 64;
        double x[kChunks];   // all loads first: they do not wait for one another
#pragma unroll
        for (int i = 0; i < kChunks; ++i) {
            const int k = i * 64 + lane;
            x[i] = k < kPqIdsPerClass ? __longlong_as_double((long long)ld64(iou_tab + c * kPqIdsPerClass + k)) : 0.0;
        }
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < kChunks; ++i) {
            u64 live = __ballot(x[i] != 0.0);
            while (live) {
                const int src = __ffsll((long long)live) - 1;
                sum += __shfl(x[i], src, 64);
                live &= live - 1;
            }
        }
        if (lane == 0) {
            row[c * 4 + 0] = sum;
            row[c * 4 + 1] = (double)cnt[c * 3 + 0];
            row[c * 4 + 2] = (double)cnt[c * 3 + 1];
            row[c * 4 + 3] = (double)cnt[c * 3 + 2];
        }
    }
}

__global__ __launch_bounds__(128) void pq_finish_kernel(PqArgs a) {
    const int t = threadIdx.x;
    const unsigned *flags = reinterpret_cast<const unsigned *>(a.ws + a.l.flags);
    const double *rows = reinterpret_cast<const double *>(a.ws + a.l.rows);
    unsigned st = 0;
    double sum = t < a.n_cls * 4 ? a.acc[t] : 0.0;
    for (int b = 0; b < a.B; ++b) {   // image order
        const unsigned f = flags[b];
        st |= f;
        if (t >= a.n_cls * 4) continue;
        const double x = f ? 0.0 : rows[(size_t)b * kPqMaxCls * 4 + t];
        sum += x;
        if (a.per_image) a.per_image[(size_t)b * a.n_cls * 4 + t] = x;
    }
    if (t < a.n_cls * 4) a.acc[t] = sum;
    if (t == 0 && st) atomicOr(reinterpret_cast<unsigned *>(a.ws), st);
}

}  // namespace pf

extern "C" int pf_pq_workspace(int B, size_t *bytes) {
    if (!bytes || B < 0) return pf::fail(PF_EINVAL, "pf_pq_workspace: bad arguments");
    *bytes = pf::pq_layout(B).total;
    return PF_OK;
}

extern "C" int pf_pq_table_slots(void) { return pf::kPqSlots; }

extern "C" int pf_pq_accumulate(const void *pred, int pred_is_i64, const void *gt, int gt_is_i64, int fmt, int crowd, int n_cls, int B,
                                int H, int W, double *acc, double *per_image, void *ws, size_t ws_bytes, void *stream) {
    if (B < 0 || H <= 0 || W <= 0 || !acc || !ws || n_cls < 1 || n_cls > pf::kPqMaxCls || fmt < 0 || fmt > 1)
        return pf::fail(PF_EINVAL, "pf_pq_accumulate: bad arguments (B=%d H=%d W=%d n_cls=%d fmt=%d)", B, H, W, n_cls, fmt);
    if (B == 0) return PF_OK;
    if (!pred || !gt) return pf::fail(PF_EINVAL, "pf_pq_accumulate: null label map");
    const size_t n = (size_t)H * W;
    if (n % 4) return pf::fail(PF_EUNSUPPORTED, "pf_pq_accumulate: H*W must be a multiple of 4");
    if (n >= ((size_t)1 << 32)) return pf::fail(PF_EUNSUPPORTED, "pf_pq_accumulate: H*W must be below 2^32 (areas are u32)");
    if (B > 65535) return pf::fail(PF_EUNSUPPORTED, "pf_pq_accumulate: B must be at most 65535");
    if (((uintptr_t)pred | (uintptr_t)gt | (uintptr_t)ws) & 15)
        return pf::fail(PF_EINVAL, "pf_pq_accumulate: pred, gt and ws must be 16-byte aligned");
    const pf::PqLayout l = pf::pq_layout(B);
    if (ws_bytes < l.total) return pf::fail(PF_EWORKSPACE, "pf_pq_accumulate: workspace %zu B < required %zu B", ws_bytes, l.total);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = pf::launch_zero_fill((char *)ws + l.flags, l.total - l.flags, s)) return rc;
    pf::PqArgs a{pred, gt, (char *)ws, l, acc, per_image, n, B, fmt, crowd ? 1 : 0, n_cls};
    const size_t trips = ((n >> 2) + pf::kPqCountThreads - 1) / pf::kPqCountThreads;
    size_t gx = (trips + pf::kPqTripsPerGroup - 1) / pf::kPqTripsPerGroup;
    gx = gx > 256 ? 256 : gx;
    const dim3 grid((unsigned)gx, (unsigned)B);
    {
        pf::ProfScope ps(s, "pf::pq_count_kernel(pf::PqArgs)", 0.0, (double)B * n * ((pred_is_i64 ? 8.0 : 4.0) + (gt_is_i64 ? 8.0 : 4.0)));
        if (pred_is_i64 && gt_is_i64) hipLaunchKernelGGL((pf::pq_count_kernel<true, true>), grid, dim3(pf::kPqCountThreads), 0, s, a);
        else if (pred_is_i64) hipLaunchKernelGGL((pf::pq_count_kernel<true, false>), grid, dim3(pf::kPqCountThreads), 0, s, a);
        else if (gt_is_i64) hipLaunchKernelGGL((pf::pq_count_kernel<false, true>), grid, dim3(pf::kPqCountThreads), 0, s, a);
        else hipLaunchKernelGGL((pf::pq_count_kernel<false, false>), grid, dim3(pf::kPqCountThreads), 0, s, a);
        PF_LAUNCH_CHECK("pq_count_kernel");
    }
    {
        pf::ProfScope ps(s, "pf::pq_match_kernel(pf::PqArgs)", 0.0, (double)B * l.image_stride);
        hipLaunchKernelGGL(pf::pq_match_kernel, dim3(B), dim3(1024), 0, s, a);
        PF_LAUNCH_CHECK("pq_match_kernel");
    }
    hipLaunchKernelGGL(pf::pq_finish_kernel, dim3(1), dim3(128), 0, s, a);
    PF_LAUNCH_CHECK("pq_finish_kernel");
    return PF_OK;
}

extern "C" int pf_pq_status(const void *ws, void *stream, int *host_status) { return pf::sticky_status_read("pf_pq_status", ws, stream, host_status); }

extern "C" int pf_pq_status_reset(void *ws, void *stream) { return pf::sticky_status_reset("pf_pq_status_reset", ws, stream); }
