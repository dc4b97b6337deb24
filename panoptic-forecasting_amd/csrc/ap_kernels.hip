// Instance AP on the device: the integer records behind AP / AP50 of the Cityscapes instance-level evaluation
// (cityscapesscripts.evaluation.evalInstanceLevelSemanticLabeling; that package is absent and unpinned: parity unpinned).  Every
// predicted mask is intersected with every ground-truth region of its label.  Integers only, enqueue only; the float64 curve is
// the host's (instance_ap.ap_from_records).  The definition stands in include/pfhip.h, pf_ap_accumulate block.
//
//   ap_size_kernel     grid (pixel chunks, B): the ground truth alone.  A lane owns kApSizeTrips consecutive units of four pixels
//                      (scan_span's head / units / tail with the map as both a and b), loads them all at once, folds runs of equal
//                      values in registers and adds a finished run of an instance label to the image's dense size table
//                      u32 [8][kApSlots] (slot k < 1000: instance k, slot 1000: the group).  Every other value leaves at once.  A
//                      value outside [0, 65536) (compared in the map's own width) sets the image's flag.
//   ap_overlap_kernel  grid (pixel chunks, P): label_scan.h's scan with the mask as map a and the prediction's image as map b.
//                      A prediction with a bad index, a label that is no instance class or a flagged image leaves at once.  Runs
//                      of equal (inside, value) are folded in registers; every pixel outside the mask folds into key 0, which
//                      leaves at once.  A run inside is classified once: group or instance of the prediction's own label, void,
//                      or neither.  The prediction sees only its own label, so the workgroup's table is dense: 1000 instances +
//                      group + void + pixels, kApPredSlots u32 = 4 KB of LDS, no hashing.  It is added to the prediction's table
//                      in the workspace when the workgroup ends.  Integer adds: the order the atomics arrive in does not matter.
//   ap_record_kernel   one wave per prediction: walks its 1001 slots against the image's size table, adds the ignore pixels, finds
//                      best (largest intersection, ties to the smaller value: group before instances, then ascending k) by a
//                      wave-wide max of (inter << 16 | 0xffff - order) and writes rec.  A flagged prediction ORs
//                      PF_AP_STATUS_INDEX into the status word.
//   ap_regular_kernel  one workgroup per image, one wave per class: counts the regular regions into gt_regular (zero for a flagged
//                      image) and ORs the image's flag into the status word.
#include "gt_labels.h"
#include "label_scan.h"
#include "pf_common.h"
#include "pf_prof.h"

namespace pf {

constexpr int kApClasses = 8;                   // labelIds 24 25 26 27 28 31 32 33 = trainIds 11..18
constexpr int kApIndices = 1000;                // k of labelId * 1000 + k
constexpr int kApSlots = 1008;                  // a class's row of the size table: 1000 instances, the group, padding to 16 B
constexpr int kApGroup = 1000, kApVoid = 1001, kApPixels = 1002;
constexpr int kApPredSlots = 1024;              // a prediction's table: instances, group, void, pixels, padding
constexpr int kApLabels = 34;                   // mask_label must be below this
constexpr int kApSizeTrips = kScanChunkPixels / 4 / kScanThreads;   // units of four pixels a lane of the size pass owns
constexpr unsigned kApDiv1000 = 4294968u;       // ceil(2^32 / 1000): __umulhi(v, .) == v / 1000 for v < 65536 (checked below)
enum { kApGtU16 = 0, kApGtI32 = 1, kApGtI64 = 2 };
enum { kApCounted = 0, kApEmpty = 1, kApNoClass = 2, kApFlagged = 3 };

constexpr unsigned ap_div1000(unsigned v) { return (unsigned)(((unsigned long long)v * kApDiv1000) >> 32); }
constexpr bool ap_div_is_exact() {   // the product is monotonic in v: the first and last value of every thousand decide
    for (unsigned q = 0; q < 66u; ++q)
        if (ap_div1000(q * 1000u) != q || ap_div1000(q * 1000u + 999u) != q) return false;
    return true;
}
static_assert(ap_div_is_exact(), "the multiplier divides every u16 value by 1000");
static_assert(kApSizeTrips * 4 * kScanThreads == kScanChunkPixels, "the size pass's lanes share a chunk evenly");

// labelId -> class index 0..7, -1: no instance class (the labels with a thing trainId, gt_labels.h)
constexpr int ap_class_of(int label) {
    if (label < 0 || label >= 64) return -1;
    const int t = kGtTrainLut.t[label];
    return (t >= kPanFirstThing && t < kPanFirstThing + kApClasses) ? t - kPanFirstThing : -1;
}
// bit v: v is the id of an ignoreInEval label (a void pixel of the instance map)
constexpr unsigned long long ap_void_mask() {
    unsigned long long m = 0;
    for (int i = 0; i < kGtLabelCount; ++i)
        if (kGtLabels[i].id >= 0 && kGtLabels[i].ignore_in_eval) m |= 1ull << kGtLabels[i].id;
    return m;
}
constexpr unsigned long long kApVoidMask = ap_void_mask();
static_assert(ap_class_of(24) == 0 && ap_class_of(28) == 4 && ap_class_of(31) == 5 && ap_class_of(33) == 7 && ap_class_of(29) == -1 &&
                  ap_class_of(23) == -1,
              "person .. bicycle are classes 0..7");
// the classes' labelIds as a device-side table (a label in [0, 34) indexes it)
struct ApClassLut {
    signed char c[64];
};
constexpr ApClassLut ap_class_lut() {
    ApClassLut l{};
    for (int i = 0; i < 64; ++i) l.c[i] = (signed char)ap_class_of(i);
    return l;
}
__device__ const ApClassLut kApClassLut = ap_class_lut();

// workspace: [0, 256) sticky status word; from 256 on everything is zeroed by every call
struct ApLayout {
    size_t flags, sizes, preds, total;
};

static ApLayout ap_layout(int P, int B) {
    ApLayout l;
    const size_t b = (size_t)(B > 0 ? B : 1), p = (size_t)(P > 0 ? P : 1);
    l.flags = 256;
    l.sizes = l.flags + align_up(b * sizeof(unsigned), 256);
    l.preds = l.sizes + align_up(b * kApClasses * kApSlots * sizeof(unsigned), 256);
    l.total = l.preds + align_up(p * kApPredSlots * sizeof(unsigned), 256);
    return l;
}

struct ApArgs {
    const unsigned char *masks;
    const int *mask_image, *mask_label;
    const void *gt;
    char *ws;
    ApLayout l;
    int *rec, *gt_regular;
    size_t n_per_image;
    int P, B, min_region;
};

template <int KIND> struct ApGt;
template <> struct ApGt<kApGtU16> { typedef unsigned short T; };
template <> struct ApGt<kApGtI32> { typedef int T; };
template <> struct ApGt<kApGtI64> { typedef long long T; };

// ---- size pass ----

// a finished run of n pixels of value v < 65536 of the ground truth
__device__ __forceinline__ void ap_size_flush(unsigned *table, unsigned v, unsigned n) {
    if (v < 1000u) {
        const int c = v < 64u ? kApClassLut.c[v] : -1;
        if (c >= 0) atomicAdd(table + c * kApSlots + kApGroup, n);
        return;
    }
    const unsigned label = __umulhi(v, kApDiv1000);   // at most 65
    const int c = label < 64u ? kApClassLut.c[label] : -1;
    if (c >= 0) atomicAdd(table + c * kApSlots + (v - label * 1000u), n);
}

struct ApSizeSink {
    unsigned *table;
    __device__ __forceinline__ void flush(unsigned v, unsigned n) { ap_size_flush(table, v, n); }
};

template <int GK>
__global__ __launch_bounds__(kScanThreads) void ap_size_kernel(ApArgs a) {
    typedef typename ApGt<GK>::T GT;
    constexpr size_t kUnitsPerChunk = kScanChunkPixels / 4;
    const int b = blockIdx.y, tid = threadIdx.x;
    const size_t n = a.n_per_image;
    const GT *g = reinterpret_cast<const GT *>(a.gt) + (size_t)b * n;
    ApSizeSink sink{reinterpret_cast<unsigned *>(a.ws + a.l.sizes) + (size_t)b * kApClasses * kApSlots};
    const ScanSpan sp = scan_span((uintptr_t)g, (uintptr_t)g, sizeof(GT), sizeof(GT), scan_align<GT, 4>(), scan_align<GT, 4>(), n, 4);
    bool ok = true;
    const size_t u1 = sp.units;
    const size_t u0 = (size_t)blockIdx.x * kUnitsPerChunk + (size_t)tid * kApSizeTrips;   // this lane's consecutive units
    unsigned v[kApSizeTrips][4];
    bool good[kApSizeTrips];
#pragma unroll
    for (int k = 0; k < kApSizeTrips; ++k) {
        good[k] = true;
        if (u0 + k < u1) good[k] = load4<GT, 16>(g, sp.head + (u0 + k) * 4, sp.al_b, v[k]);
    }
    RunFold f{0u, 0u};
#pragma unroll
    for (int k = 0; k < kApSizeTrips; ++k) {
        if (u0 + k >= u1) continue;
        if (!good[k]) {   // the image is flagged and adds nothing: its pixels need not be counted
            ok = false;
            continue;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) fold_pixel(f, sink, v[k][j]);
    }
    if (f.run) sink.flush(f.cur, f.run);
    if (blockIdx.x == 0) {   // head and tail, one lane per pixel: fewer than 16 + 4 of them
        const size_t ntail = n - sp.tail0;
        size_t i = n;
        if ((size_t)tid < sp.head) i = tid;
        else if ((size_t)tid - sp.head < ntail) i = sp.tail0 + ((size_t)tid - sp.head);
        if (i < n) {
            unsigned x;
            if (load1<GT, 16>(g, i, x)) sink.flush(x, 1u);
            else ok = false;
        }
    }
    if (!ok) atomicOr(reinterpret_cast<unsigned *>(a.ws + a.l.flags) + b, PF_AP_STATUS_VALUE);
}

// ---- overlap pass ----

// the sink of the scan; key = value << 8 | mask byte, and every pixel outside the mask is key 0 where the sink builds the key
struct ApFold {
    unsigned *tab;        // the workgroup's table in LDS
    unsigned label;       // the prediction's labelId
    unsigned pixels;      // this lane's pixels inside the mask
    unsigned mc, gc;      // u8 x u16 path: the mask word / value pair of four pixels that continue the fold's current run

    __device__ __forceinline__ void flush(unsigned key, unsigned n) {
        if (!(key & 255u)) return;   // outside the mask: almost every run
        pixels += n;
        const unsigned v = key >> 8;
        if (v < 1000u) {
            if (v == label) atomicAdd(tab + kApGroup, n);
            else if (v < 64u && ((kApVoidMask >> v) & 1ull)) atomicAdd(tab + kApVoid, n);
            return;
        }
        const unsigned l = __umulhi(v, kApDiv1000);
        if (l == label) atomicAdd(tab + (v - l * 1000u), n);
    }

    // four pixels: a word of mask bytes and two words of value halves
    __device__ __forceinline__ void word(RunFold &f, unsigned mw, unsigned g0, unsigned g1) {
        if (mw == 0u) {   // all four outside
            if (f.cur == 0u) {
                f.run += 4;
            } else {
                fold_pixel(f, *this, 0u);
                f.run += 3;
                mc = 0u;
            }
            return;
        }
        if (mw == mc && g0 == gc && g1 == gc) {
            f.run += 4;
            return;
        }
        fold_pixel(f, *this, (mw & 255u) ? ((g0 & 65535u) << 8) | 1u : 0u);
        fold_pixel(f, *this, ((mw >> 8) & 255u) ? ((g0 >> 16) << 8) | 1u : 0u);
        fold_pixel(f, *this, ((mw >> 16) & 255u) ? ((g1 & 65535u) << 8) | 1u : 0u);
        fold_pixel(f, *this, (mw >> 24) ? ((g1 >> 16) << 8) | 1u : 0u);
        // the next word continues the run when it is this word again and this word is one run that is inside
        const bool inside4 = ((((mw & 0x7f7f7f7fu) + 0x7f7f7f7fu) | mw) & 0x80808080u) == 0x80808080u;
        const bool one = g0 == g1 && (g0 >> 16) == (g0 & 65535u);
        mc = (inside4 && one) ? mw : 0u;
        gc = g0;
    }

    __device__ __forceinline__ void raw(RunFold &f, const uint4 &m, const uint4 (&g)[2]) {
        word(f, m.x, g[0].x, g[0].y);
        word(f, m.y, g[0].z, g[0].w);
        word(f, m.z, g[1].x, g[1].y);
        word(f, m.w, g[1].z, g[1].w);
    }
};

template <int GK>
__global__ __launch_bounds__(kScanThreads) void ap_overlap_kernel(ApArgs a) {
    typedef typename ApGt<GK>::T GT;
    constexpr int P = GK == kApGtU16 ? 16 : 4;   // pixels of one unit
    __shared__ unsigned tab[kApPredSlots];
    const int p = blockIdx.y, tid = threadIdx.x;
    const int image = a.mask_image[p], label = a.mask_label[p];
    if (image < 0 || image >= a.B || label < 0 || label >= kApLabels) return;   // the whole workgroup: flagged by ap_record_kernel
    if (kApClassLut.c[label] < 0) return;
    if (reinterpret_cast<const unsigned *>(a.ws + a.l.flags)[image]) return;   // set by the size pass, which has ended
    for (int i = tid; i < kApPredSlots; i += kScanThreads) tab[i] = 0u;
    __syncthreads();

    const size_t n = a.n_per_image;
    const unsigned char *mb = a.masks + (size_t)p * n;
    const GT *gb = reinterpret_cast<const GT *>(a.gt) + (size_t)image * n;
    ApFold sink{tab, (unsigned)label, 0u, 0u, 0u};
    label_scan<unsigned char, GT, 16, P>(mb, gb, n, sink);   // a value out of range was met by the size pass too
    if (sink.pixels) atomicAdd(tab + kApPixels, sink.pixels);
    __syncthreads();
    unsigned *mine = reinterpret_cast<unsigned *>(a.ws + a.l.preds) + (size_t)p * kApPredSlots;
    for (int i = tid; i <= kApPixels; i += kScanThreads)
        if (tab[i]) atomicAdd(mine + i, tab[i]);
}

// ---- finish ----

__global__ __launch_bounds__(64) void ap_record_kernel(ApArgs a) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int image = a.mask_image[p], label = a.mask_label[p];
    int *rec = a.rec + (size_t)p * 8;
    const bool bad = image < 0 || image >= a.B || label < 0 || label >= kApLabels;
    const int cls = bad ? -1 : kApClassLut.c[label];
    int state = kApCounted;
    if (bad) state = kApFlagged;
    else if (reinterpret_cast<const unsigned *>(a.ws + a.l.flags)[image]) state = kApFlagged;
    else if (cls < 0) state = kApNoClass;
    unsigned pixels = 0, ignore = 0, best_inter = 0, best_pixels = 0;
    int best_value = -1;
    if (state == kApCounted) {
        const unsigned *mine = reinterpret_cast<const unsigned *>(a.ws + a.l.preds) + (size_t)p * kApPredSlots;
        const unsigned *size = reinterpret_cast<const unsigned *>(a.ws + a.l.sizes) + ((size_t)image * kApClasses + cls) * kApSlots;
        pixels = mine[kApPixels];
        if (pixels == 0u) {
            state = kApEmpty;
        } else {
            const unsigned min_region = (unsigned)a.min_region;
            unsigned long long best = 0ull;   // inter << 16 | 0xffff - order; order 0: the group, k + 1: instance k
            unsigned ign = 0u;
            constexpr int kSteps = (kApGroup + 1 + 63) / 64;
            unsigned in[kSteps], sz[kSteps];
#pragma unroll
            for (int s = 0; s < kSteps; ++s) {
                const int k = s * 64 + lane;
                in[s] = k <= kApGroup ? mine[k] : 0u;
                sz[s] = k <= kApGroup ? size[k] : 0u;
            }
#pragma unroll
            for (int s = 0; s < kSteps; ++s) {
                const int k = s * 64 + lane;
                if (in[s] == 0u) continue;
                if (k == kApGroup) ign += in[s];
                if (sz[s] < min_region) ign += in[s];   // a small group is added twice, as in the original
                const unsigned order = k == kApGroup ? 0u : (unsigned)k + 1u;
                const unsigned long long cand = ((unsigned long long)in[s] << 16) | (0xffffu - order);
                best = cand > best ? cand : best;
            }
            for (int d = 32; d > 0; d >>= 1) {
                const unsigned long long o = __shfl_xor(best, d);
                best = o > best ? o : best;
                ign += __shfl_xor(ign, d);
            }
            ignore = ign + mine[kApVoid];
            if (best) {
                const unsigned order = 0xffffu - (unsigned)(best & 0xffffull);
                const int slot = order == 0u ? kApGroup : (int)order - 1;
                best_inter = (unsigned)(best >> 16);
                best_pixels = size[slot];
                best_value = order == 0u ? label : label * 1000 + slot;
            }
        }
    }
    if (lane == 0) {
        rec[0] = state;
        rec[1] = (int)pixels;
        rec[2] = (int)ignore;
        rec[3] = best_value;
        rec[4] = (int)best_inter;
        rec[5] = (int)best_pixels;
        rec[6] = image;
        rec[7] = cls;
        if (bad) atomicOr(reinterpret_cast<unsigned *>(a.ws), PF_AP_STATUS_INDEX);
    }
}

__global__ __launch_bounds__(kApClasses * 64) void ap_regular_kernel(ApArgs a) {
    const int b = blockIdx.x, cls = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned flag = reinterpret_cast<const unsigned *>(a.ws + a.l.flags)[b];
    const unsigned *size = reinterpret_cast<const unsigned *>(a.ws + a.l.sizes) + ((size_t)b * kApClasses + cls) * kApSlots;
    const unsigned min_region = (unsigned)a.min_region;
    int count = 0;
    for (int k = lane; k < kApIndices; k += 64) {
        const unsigned s = size[k];
        count += (s != 0u && s >= min_region) ? 1 : 0;
    }
    for (int d = 32; d > 0; d >>= 1) count += __shfl_xor(count, d);
    if (lane == 0) a.gt_regular[(size_t)b * kApClasses + cls] = flag ? 0 : count;
    if (threadIdx.x == 0 && flag) atomicOr(reinterpret_cast<unsigned *>(a.ws), flag);
}

template <typename K>
static void ap_launch(K size_or_overlap_u16, K i32, K i64, int gt_kind, dim3 grid, hipStream_t s, const ApArgs &a) {
    K k = gt_kind == kApGtU16 ? size_or_overlap_u16 : gt_kind == kApGtI32 ? i32 : i64;
    hipLaunchKernelGGL(k, grid, dim3(kScanThreads), 0, s, a);
}

}  // namespace pf

extern "C" int pf_ap_workspace(int P, int B, size_t *bytes) {
    if (!bytes || P < 0 || B < 0) return pf::fail(PF_EINVAL, "pf_ap_workspace: bad arguments");
    *bytes = pf::ap_layout(P, B).total;
    return PF_OK;
}

extern "C" int pf_ap_chunk_pixels(void) { return pf::kScanChunkPixels; }

extern "C" int pf_debug_ap_slot(int value, int label, int *slot) {
    if (!slot || value < 0 || value > 65535 || label < 0 || label >= pf::kApLabels)
        return pf::fail(PF_EINVAL, "pf_debug_ap_slot: null output, a value outside [0, 65536) or a label outside [0, 34)");
    *slot = -1;   // neither
    if (pf::ap_class_of(label) < 0) return PF_OK;
    if (value < 1000) {
        if (value == label) *slot = pf::kApGroup;
        else if (value < 64 && ((pf::kApVoidMask >> value) & 1ull)) *slot = pf::kApVoid;
    } else if ((int)pf::ap_div1000((unsigned)value) == label) {
        *slot = value - label * 1000;
    }
    return PF_OK;
}

extern "C" int pf_ap_accumulate(const void *masks, const int *mask_image, const int *mask_label, int P, const void *gt, int gt_kind,
                                int B, int H, int W, int min_region, int *rec, int *gt_regular, void *ws, size_t ws_bytes, void *stream) {
    if (P < 0 || B < 0 || H <= 0 || W <= 0 || !ws || gt_kind < 0 || gt_kind > 2 || min_region < 0)
        return pf::fail(PF_EINVAL, "pf_ap_accumulate: bad arguments (P=%d B=%d H=%d W=%d gt_kind=%d min_region=%d)", P, B, H, W, gt_kind,
                        min_region);
    if (P == 0 && B == 0) return PF_OK;
    if (P > 0 && (!masks || !mask_image || !mask_label || !rec)) return pf::fail(PF_EINVAL, "pf_ap_accumulate: null masks, mask_image, mask_label or rec");
    if (B > 0 && (!gt || !gt_regular)) return pf::fail(PF_EINVAL, "pf_ap_accumulate: null gt or gt_regular");
    const size_t n = (size_t)H * W;
    if (n >= ((size_t)1 << 30)) return pf::fail(PF_EUNSUPPORTED, "pf_ap_accumulate: H*W must be below 2^30 (rec holds i32 pixel counts; ignore is at most twice the mask)");
    if (B > 65535 || P > 65535) return pf::fail(PF_EUNSUPPORTED, "pf_ap_accumulate: P and B must be at most 65535");
    const size_t gsz[3] = {2, 4, 8};
    if ((uintptr_t)gt % gsz[gt_kind]) return pf::fail(PF_EINVAL, "pf_ap_accumulate: gt must be aligned to its element size");
    if (((uintptr_t)ws & 15) || ((uintptr_t)rec & 3) || ((uintptr_t)gt_regular & 3) || ((uintptr_t)mask_image & 3) || ((uintptr_t)mask_label & 3))
        return pf::fail(PF_EINVAL, "pf_ap_accumulate: ws must be 16-byte aligned, the i32 arrays 4-byte aligned");
    const pf::ApLayout l = pf::ap_layout(P, B);
    if (ws_bytes < l.total) return pf::fail(PF_EWORKSPACE, "pf_ap_accumulate: workspace %zu B < required %zu B", ws_bytes, l.total);
    hipStream_t s = (hipStream_t)stream;
    pf::ApArgs a{(const unsigned char *)masks, mask_image, mask_label, gt, (char *)ws, l, rec, gt_regular, n, P, B, min_region};
    const size_t gx = (n + pf::kScanChunkPixels - 1) / pf::kScanChunkPixels;   // the units are at most n pixels; at least one workgroup
    if (B > 0) {
        if (int rc = pf::launch_zero_fill((char *)ws + l.flags, l.total - l.flags, s)) return rc;
        pf::ProfScope ps(s, "pf::ap_size_kernel(pf::ApArgs)", 0.0, (double)B * n * (double)gsz[gt_kind]);
        pf::ap_launch(pf::ap_size_kernel<pf::kApGtU16>, pf::ap_size_kernel<pf::kApGtI32>, pf::ap_size_kernel<pf::kApGtI64>, gt_kind,
                      dim3((unsigned)gx, (unsigned)B), s, a);
        PF_LAUNCH_CHECK("ap_size_kernel");
    }
    if (B > 0 && P > 0) {
        pf::ProfScope ps(s, "pf::ap_overlap_kernel(pf::ApArgs)", 0.0, (double)P * n * (double)(1 + gsz[gt_kind]));
        pf::ap_launch(pf::ap_overlap_kernel<pf::kApGtU16>, pf::ap_overlap_kernel<pf::kApGtI32>, pf::ap_overlap_kernel<pf::kApGtI64>, gt_kind,
                      dim3((unsigned)gx, (unsigned)P), s, a);
        PF_LAUNCH_CHECK("ap_overlap_kernel");
    }
    if (P > 0) {   // with B == 0 every prediction's index is out of range: nothing of the workspace but the status word is read
        pf::ProfScope ps(s, "pf::ap_record_kernel(pf::ApArgs)", 0.0, (double)P * pf::kApPredSlots * 8.0);
        hipLaunchKernelGGL(pf::ap_record_kernel, dim3((unsigned)P), dim3(64), 0, s, a);
        PF_LAUNCH_CHECK("ap_record_kernel");
    }
    if (B > 0) {
        pf::ProfScope ps(s, "pf::ap_regular_kernel(pf::ApArgs)", 0.0, (double)B * pf::kApClasses * pf::kApSlots * 4.0);
        hipLaunchKernelGGL(pf::ap_regular_kernel, dim3((unsigned)B), dim3(pf::kApClasses * 64), 0, s, a);
        PF_LAUNCH_CHECK("ap_regular_kernel");
    }
    return PF_OK;
}

extern "C" int pf_ap_status(const void *ws, void *stream, int *host_status) {
    return pf::sticky_status_read("pf_ap_status", ws, stream, host_status);
}

extern "C" int pf_ap_status_reset(void *ws, void *stream) { return pf::sticky_status_reset("pf_ap_status_reset", ws, stream); }
