// Cityscapes ground-truth preparation on the device: one pass over the instance maps (*_gtFine_instanceIds.png: a value below 1000 is
// a labelId, any other labelId * 1000 + instance index) gives the panoptic PNG's pixels, the trainId map, the trainId map without
// the thing classes and each image's segment list {v, area, x, y, width, height} - what createPanopticImgs,
// createTrainIdLabelImgs (cityscapesscripts.preparation; absent and unpinned: parity unpinned) and the reference's
// scripts/preprocessing/remove_fg_from_gt.py compute.  Integers only.  Enqueue only.
//
//   gt_stream_kernel   grid (pixel chunks of kGtChunkPixels, B), a chunk never spans two images.  An image of n pixels is
//                      [head | units | tail]: the head ends where the OUTPUTS of the image reach a unit's alignment (pixel b * n + head
//                      is a multiple of P; the output bases are 16-byte aligned), a unit is P pixels (8 of a u16 map: one 16-byte
//                      load; 4 of an i32 / i64 map).  Where the instance map is not 16-byte aligned at that pixel its units are read
//                      by element loads: slower, never refused.  A lane loads kGtGroup units at once and writes per unit P
//                      trainId bytes, P no-foreground bytes and 3 P colour bytes as whole words.  It keeps one segment in
//                      registers - value, area, x and y extents; its consecutive units lie 256 * P pixels apart, one below the other
//                      in a 2048-wide image - and while a unit repeats that value inside one row the unit costs one compare per word,
//                      five updates and the stores of words splatted from the value's class.  A value that ends is added to the
//                      workgroup's table in LDS (kGtLdsSlots entries, open addressing, kGtProbes probes; integer add / max
//                      atomics, minima kept as maxima of the complement so that zero means empty), past that straight to the
//                      image's table.  Segments of ignoreInEval labels are dropped there.  The LDS entries are added to the
//                      image's dense table in the workspace when the workgroup ends.  Head and tail go through per element
//                      (workgroup 0 of the image, one lane per pixel).  An illegal value flags the image; its own pixels are
//                      written as void (black, 255).
//   gt_finish_kernel   one workgroup of 1024 per image: walks the area column of the dense table 1024 slots at a time (slot order is
//                      ascending v), ranks the non-empty slots by ballots and a scan over the (step, wave) counts, and writes
//                      the rows in that order.  A flagged image and an image with more segments than the list holds get
//                      seg_count 0; the flags are ORed into the sticky status word.
// Dense table, not a hash table: 34 + 33 * 1000 slots cover every legal value, slot order is value order, so the finish pass is a
// compaction, not a sort, and no image can overflow the table itself.
#include "gt_labels.h"
#include "label_scan.h"
#include "pf_common.h"
#include "pf_prof.h"

namespace pf {

constexpr int kGtThreads = 256;
constexpr int kGtChunkPixels = 16384;          // pixels of units one stream workgroup owns, whatever the kind
constexpr int kGtGroup = 4;                    // units whose loads are in flight together
constexpr int kGtSlots = 34 + 33 * 1000;       // v < 1000: slot v (34 legal ones); v >= 1000: slot 34 + v - 1000
constexpr int kGtFields = 5;                   // columns of the dense table: area, ~xmin, xmax, ~ymin, ymax
constexpr int kGtMaxSegments = 1024;           // rows of an image's segment list
constexpr int kGtLdsBits = 9;
constexpr int kGtLdsSlots = 1 << kGtLdsBits;
constexpr int kGtProbes = 4;
constexpr unsigned kGtEmpty = 0xffffffffu;
constexpr unsigned kGtNone = 0xfffffffeu;      // no value yet (a lane's fold before its first pixel)
constexpr unsigned kGtIllegal = 0xffffffffu;   // what a value outside the map's 16 low bits is decoded to
constexpr unsigned kGtDiv1000 = 4294968u;      // ceil(2^32 / 1000): __umulhi(v, .) == v / 1000 for v < 65536
constexpr int kGtFinishThreads = 1024;
constexpr int kGtFinishSteps = (kGtSlots + kGtFinishThreads - 1) / kGtFinishThreads;
enum { kGtInstU16 = 0, kGtInstI32 = 1, kGtInstI64 = 2 };

constexpr bool gt_div_is_exact() {
    for (unsigned q = 0; q < 66u; ++q)
        for (unsigned r = 0; r < 1000u; r += 999u)
            if ((unsigned)(((unsigned long long)(q * 1000u + r) * kGtDiv1000) >> 32) != q) return false;
    return true;
}
static_assert(gt_div_is_exact(), "the multiplier divides every u16 value by 1000");
static_assert(kGtFinishSteps * (kGtFinishThreads / 64) <= kGtFinishThreads, "one thread per (step, wave) count in the scan");

__device__ const GtTrainLut kGtTrainLutDev = kGtTrainLut;

// workspace: [0, 256) sticky status word; from 256 on everything is zeroed by every call
struct GtLayout {
    size_t flags, tables, total;
};

static GtLayout gt_layout(int B) {
    GtLayout l;
    const size_t b = (size_t)(B > 0 ? B : 1);
    l.flags = 256;
    l.tables = l.flags + align_up(b * sizeof(unsigned), 256);
    l.total = l.tables + align_up(b * kGtFields * kGtSlots * sizeof(unsigned), 256);
    return l;
}

struct GtArgs {
    const void *inst;
    char *ws;
    GtLayout l;
    uint8_t *rgb, *train, *nofg;
    int *seg_count, *segs;
    unsigned n;
    int B, W;
};

template <int KIND> struct GtInst;
template <> struct GtInst<kGtInstU16> { typedef unsigned short T; };
template <> struct GtInst<kGtInstI32> { typedef int T; };
template <> struct GtInst<kGtInstI64> { typedef long long T; };

// a value's class in one word: trainId byte << 24 | the 24 colour bits (the value itself; 0 for a label without a trainId).
// An illegal value is void too; *bad is set.
__device__ __forceinline__ unsigned gt_classify(unsigned v, const unsigned char *lut, bool &bad) {
    const bool legal = v < 34u || (v - 1000u) < 33000u;
    if (!legal) bad = true;
    const unsigned label = v < 1000u ? v : __umulhi(v, kGtDiv1000);
    const unsigned train = lut[legal ? label : 0u];
    return (train << 24) | (train == 255u ? 0u : v);
}

__device__ __forceinline__ unsigned gt_nofg(unsigned train) { return (train - (unsigned)kPanFirstThing) < 8u ? 255u : train; }

// a workgroup's table in LDS and the image's dense table in the workspace
struct GtTables {
    unsigned *key;     // [kGtLdsSlots] slot or kGtEmpty
    unsigned *val;     // [kGtLdsSlots][kGtFields]
    unsigned *image;   // [kGtFields][kGtSlots]; null: the call lists no segments
};

__device__ __forceinline__ void gt_add(const GtTables &t, unsigned slot, unsigned area, unsigned xmin, unsigned xmax, unsigned ymin,
                                       unsigned ymax) {
    unsigned h = (slot * 0x9E3779B1u) >> (32 - kGtLdsBits);
#pragma unroll 1
    for (int probe = 0; probe < kGtProbes; ++probe) {
        const unsigned old = atomicCAS(t.key + h, kGtEmpty, slot);
        if (old == kGtEmpty || old == slot) {
            unsigned *e = t.val + kGtFields * h;
            atomicAdd(e, area);
            atomicMax(e + 1, ~xmin);
            atomicMax(e + 2, xmax);
            atomicMax(e + 3, ~ymin);
            atomicMax(e + 4, ymax);
            return;
        }
        h = (h + 1) & (kGtLdsSlots - 1);
    }
    atomicAdd(t.image + slot, area);
    atomicMax(t.image + kGtSlots + slot, ~xmin);
    atomicMax(t.image + 2 * kGtSlots + slot, xmax);
    atomicMax(t.image + 3 * kGtSlots + slot, ~ymin);
    atomicMax(t.image + 4 * kGtSlots + slot, ymax);
}

// the segment a lane holds in registers
struct GtFold {
    unsigned cur, pk;   // value, its class word
    unsigned area, xmin, xmax, ymin, ymax;
    bool bad;
};

__device__ __forceinline__ void gt_flush(const GtFold &f, const GtTables &t) {
    if (!f.area || !t.image || (f.pk >> 24) == 255u) return;   // nothing held / no list wanted / ignoreInEval or illegal
    gt_add(t, f.cur < 1000u ? f.cur : f.cur - 1000u + 34u, f.area, f.xmin, f.xmax, f.ymin, f.ymax);
}

__device__ __forceinline__ void gt_pixel(GtFold &f, const GtTables &t, const unsigned char *lut, unsigned v, unsigned x, unsigned y) {
    if (v != f.cur) {
        gt_flush(f, t);
        f.cur = v;
        f.pk = gt_classify(v, lut, f.bad);
        f.area = 0;
        f.xmin = f.ymin = 0xffffffffu;
        f.xmax = f.ymax = 0;
    }
    ++f.area;
    f.xmin = min(f.xmin, x);
    f.xmax = max(f.xmax, x);
    f.ymin = min(f.ymin, y);
    f.ymax = max(f.ymax, y);
}

// Four pixels from (x, y) on: folds them and forms their output words - tw: trainId bytes, nw: no-foreground bytes, c[3]: colours.
__device__ __forceinline__ void gt_four(GtFold &f, const GtTables &t, const unsigned char *lut, const unsigned v[4], unsigned &x,
                                        unsigned &y, unsigned W, unsigned &tw, unsigned &nw, unsigned c[3]) {
    if (v[0] == f.cur && v[1] == f.cur && v[2] == f.cur && v[3] == f.cur && x + 4u <= W) {   // the held segment goes on in this row
        const unsigned tr = f.pk >> 24, col = f.pk & 0xffffffu;
        f.area += 4;
        f.xmin = min(f.xmin, x);
        f.xmax = max(f.xmax, x + 3u);
        f.ymin = min(f.ymin, y);
        f.ymax = max(f.ymax, y);
        tw = tr * 0x01010101u;
        nw = gt_nofg(tr) * 0x01010101u;
        c[0] = col | (col << 24);
        c[1] = (col >> 8) | (col << 16);
        c[2] = (col >> 16) | (col << 8);
        x += 4u;
        if (x == W) {
            x = 0;
            ++y;
        }
        return;
    }
    unsigned col[4];
    tw = nw = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        gt_pixel(f, t, lut, v[j], x, y);
        const unsigned tr = f.pk >> 24;
        tw |= tr << (8 * j);
        nw |= gt_nofg(tr) << (8 * j);
        col[j] = f.pk & 0xffffffu;
        if (++x == W) {
            x = 0;
            ++y;
        }
    }
    c[0] = col[0] | (col[1] << 24);
    c[1] = (col[1] >> 8) | (col[2] << 16);
    c[2] = (col[2] >> 16) | (col[3] << 8);
}

// P decoded values of a unit; a value outside [0, 65536) (compared in the map's own width) becomes kGtIllegal
template <typename T, int P>
__device__ __forceinline__ void gt_load_unit(const T *base, size_t i, bool aligned, unsigned v[P]) {
    if constexpr (sizeof(T) == 2) {
        static_assert(P == 8, "a unit of a u16 map is one 16-byte load");
        const uint4 w = load_words(base, i, aligned);
        v[0] = w.x & 65535u; v[1] = w.x >> 16; v[2] = w.y & 65535u; v[3] = w.y >> 16;
        v[4] = w.z & 65535u; v[5] = w.z >> 16; v[6] = w.w & 65535u; v[7] = w.w >> 16;
    } else {
        static_assert(P == 4, "a unit of an i32 / i64 map is four pixels");
        if (!load4<T, 16>(base, i, aligned, v)) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (!load1<T, 16>(base, i + k, v[k])) v[k] = kGtIllegal;
        }
    }
}

template <int IK>
__global__ __launch_bounds__(kGtThreads) void gt_stream_kernel(GtArgs a) {
    typedef typename GtInst<IK>::T IT;
    constexpr int P = IK == kGtInstU16 ? 8 : 4;
    constexpr unsigned kUnitsPerChunk = kGtChunkPixels / P;
    static_assert(kUnitsPerChunk % (kGtGroup * kGtThreads) == 0, "a chunk is whole groups of units");

    __shared__ unsigned key[kGtLdsSlots];
    __shared__ unsigned val[kGtLdsSlots * kGtFields];
    __shared__ unsigned char lut[64];
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < kGtLdsSlots; i += kGtThreads) key[i] = kGtEmpty;
    for (int i = tid; i < kGtLdsSlots * kGtFields; i += kGtThreads) val[i] = 0;
    if (tid < 64) lut[tid] = kGtTrainLutDev.t[tid];
    __syncthreads();

    const unsigned n = a.n, W = (unsigned)a.W;
    const size_t g0 = (size_t)b * n;   // the image's first pixel in the batch
    const IT *ib = reinterpret_cast<const IT *>(a.inst) + g0;
    const bool lists = a.segs != nullptr;
    const GtTables t{key, val, lists ? reinterpret_cast<unsigned *>(a.ws + a.l.tables) + (size_t)b * kGtFields * kGtSlots : nullptr};
    unsigned head = (unsigned)((P - g0 % P) % P);
    if (head > n) head = n;
    const unsigned units = (n - head) / P, tail0 = head + units * P;
    const bool aligned = ((uintptr_t)(ib + head) & 15) == 0;

    GtFold f{kGtNone, 255u << 24, 0u, 0u, 0u, 0u, 0u, false};
    const unsigned u0 = blockIdx.x * kUnitsPerChunk;
    const unsigned u1 = u0 + kUnitsPerChunk < units ? u0 + kUnitsPerChunk : units;
    for (unsigned tu = u0; tu < u1; tu += kGtGroup * kGtThreads) {
        unsigned v[kGtGroup][P];
#pragma unroll
        for (int k = 0; k < kGtGroup; ++k) {
            const unsigned u = tu + k * kGtThreads + tid;
            if (u < u1) gt_load_unit<IT, P>(ib, head + (size_t)u * P, aligned, v[k]);
        }
#pragma unroll
        for (int k = 0; k < kGtGroup; ++k) {
            const unsigned u = tu + k * kGtThreads + tid;
            if (u >= u1) continue;
            const unsigned i = head + u * P;
            unsigned y = i / W, x = i - y * W;
            const size_t g = g0 + i;   // a multiple of P
            unsigned tw[P / 4], nw[P / 4], c[P / 4][3];
#pragma unroll
            for (int q = 0; q < P / 4; ++q) gt_four(f, t, lut, &v[k][4 * q], x, y, W, tw[q], nw[q], c[q]);
            if constexpr (P == 8) {
                if (a.train) *reinterpret_cast<uint2 *>(a.train + g) = uint2{tw[0], tw[1]};
                if (a.nofg) *reinterpret_cast<uint2 *>(a.nofg + g) = uint2{nw[0], nw[1]};
                if (a.rgb) {
                    uint2 *o = reinterpret_cast<uint2 *>(a.rgb + 3 * g);
                    o[0] = uint2{c[0][0], c[0][1]};
                    o[1] = uint2{c[0][2], c[1][0]};
                    o[2] = uint2{c[1][1], c[1][2]};
                }
            } else {
                if (a.train) *reinterpret_cast<unsigned *>(a.train + g) = tw[0];
                if (a.nofg) *reinterpret_cast<unsigned *>(a.nofg + g) = nw[0];
                if (a.rgb) {
                    unsigned *o = reinterpret_cast<unsigned *>(a.rgb + 3 * g);
                    o[0] = c[0][0];
                    o[1] = c[0][1];
                    o[2] = c[0][2];
                }
            }
        }
    }
    gt_flush(f, t);
    if (blockIdx.x == 0) {   // head and tail, one lane per pixel: fewer than 2 P <= 16 of them
        const unsigned ntail = n - tail0;
        unsigned i = n;
        if ((unsigned)tid < head) i = tid;
        else if ((unsigned)tid - head < ntail) i = tail0 + ((unsigned)tid - head);
        if (i < n) {
            unsigned v;
            if (!load1<IT, 16>(ib, i, v)) v = kGtIllegal;
            GtFold one{kGtNone, 255u << 24, 0u, 0u, 0u, 0u, 0u, false};
            const unsigned y = i / W;
            gt_pixel(one, t, lut, v, i - y * W, y);
            gt_flush(one, t);
            f.bad = f.bad || one.bad;
            const unsigned tr = one.pk >> 24, col = one.pk & 0xffffffu;
            const size_t g = g0 + i;
            if (a.train) a.train[g] = (uint8_t)tr;
            if (a.nofg) a.nofg[g] = (uint8_t)gt_nofg(tr);
            if (a.rgb) {
                a.rgb[3 * g] = (uint8_t)col;
                a.rgb[3 * g + 1] = (uint8_t)(col >> 8);
                a.rgb[3 * g + 2] = (uint8_t)(col >> 16);
            }
        }
    }
    if (f.bad) atomicOr(reinterpret_cast<unsigned *>(a.ws + a.l.flags) + b, PF_GTPREP_STATUS_VALUE);
    if (!lists) return;
    __syncthreads();
    for (int i = tid; i < kGtLdsSlots; i += kGtThreads) {
        const unsigned slot = key[i];
        if (slot == kGtEmpty) continue;
        const unsigned *e = val + kGtFields * i;
        atomicAdd(t.image + slot, e[0]);
#pragma unroll
        for (int k = 1; k < kGtFields; ++k) atomicMax(t.image + k * kGtSlots + slot, e[k]);
    }
}

__global__ __launch_bounds__(kGtFinishThreads) void gt_finish_kernel(GtArgs a) {
    constexpr int kWaves = kGtFinishThreads / 64, kCounts = kGtFinishSteps * kWaves;
    __shared__ unsigned count[kGtFinishThreads];   // per (step, wave): its non-empty slots, then their first row
    __shared__ unsigned wave_sum[kWaves];
    __shared__ unsigned total_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned flag = reinterpret_cast<const unsigned *>(a.ws + a.l.flags)[b];
    if (!a.segs) {
        if (tid == 0 && flag) atomicOr(reinterpret_cast<unsigned *>(a.ws), flag);
        return;
    }
    const unsigned *table = reinterpret_cast<const unsigned *>(a.ws + a.l.tables) + (size_t)b * kGtFields * kGtSlots;
    unsigned long long nz = 0;   // bit j: slot j * 1024 + tid is not empty (the loads are independent: issued together)
#pragma unroll
    for (int j = 0; j < kGtFinishSteps; ++j) {
        const int slot = j * kGtFinishThreads + tid;
        const unsigned area = slot < kGtSlots ? table[slot] : 0u;
        nz |= (unsigned long long)(area != 0u) << j;
    }
    count[tid] = 0;
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < kGtFinishSteps; ++j) {
        const unsigned long long m = __ballot((nz >> j) & 1ull);
        if (lane == 0) count[j * kWaves + wave] = (unsigned)__popcll(m);
    }
    __syncthreads();
    // exclusive scan of the kCounts counts in (step, wave) order = slot order
    const unsigned mine = tid < kCounts ? count[tid] : 0u;
    unsigned incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    unsigned before = 0;
    for (int w = 0; w < wave; ++w) before += wave_sum[w];
    if (tid == kGtFinishThreads - 1) total_s = before + incl;
    __syncthreads();   // every count has been read
    count[tid] = before + incl - mine;
    __syncthreads();
    const unsigned total = total_s;
    if (total > (unsigned)kGtMaxSegments) flag |= PF_GTPREP_STATUS_FULL;
    if (tid == 0) {
        a.seg_count[b] = flag ? 0 : (int)total;
        if (flag) atomicOr(reinterpret_cast<unsigned *>(a.ws), flag);
    }
    if (flag) return;
    int *rows = a.segs + (size_t)b * kGtMaxSegments * 6;
#pragma unroll 1
    for (int j = 0; j < kGtFinishSteps; ++j) {
        const unsigned long long m = __ballot((nz >> j) & 1ull);
        if ((nz >> j) & 1ull) {
            const int slot = j * kGtFinishThreads + tid;
            const unsigned row = count[j * kWaves + wave] + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            const unsigned x = ~table[kGtSlots + slot], xmax = table[2 * kGtSlots + slot];
            const unsigned y = ~table[3 * kGtSlots + slot], ymax = table[4 * kGtSlots + slot];
            int *r = rows + (size_t)row * 6;
            r[0] = slot < 34 ? slot : slot - 34 + 1000;
            r[1] = (int)table[slot];
            r[2] = (int)x;
            r[3] = (int)y;
            r[4] = (int)(xmax - x + 1u);
            r[5] = (int)(ymax - y + 1u);
        }
    }
}

}  // namespace pf

extern "C" int pf_gt_prepare_workspace(int B, size_t *bytes) {
    if (!bytes || B < 0) return pf::fail(PF_EINVAL, "pf_gt_prepare_workspace: bad arguments");
    *bytes = pf::gt_layout(B).total;
    return PF_OK;
}

extern "C" int pf_gt_prepare_max_segments(void) { return pf::kGtMaxSegments; }

extern "C" int pf_gt_prepare(const void *inst, int inst_kind, int B, int H, int W, uint8_t *out_rgb, uint8_t *out_train,
                             uint8_t *out_train_nofg, int *seg_count, int *segs, void *ws, size_t ws_bytes, void *stream) {
    if (B < 0 || H <= 0 || W <= 0 || !ws || inst_kind < 0 || inst_kind > 2)
        return pf::fail(PF_EINVAL, "pf_gt_prepare: bad arguments (B=%d H=%d W=%d inst_kind=%d)", B, H, W, inst_kind);
    if ((seg_count == nullptr) != (segs == nullptr)) return pf::fail(PF_EINVAL, "pf_gt_prepare: seg_count and segs go together");
    if (B == 0) return PF_OK;
    if (!inst) return pf::fail(PF_EINVAL, "pf_gt_prepare: null map");
    const size_t n = (size_t)H * W;
    if (n >= ((size_t)1 << 31)) return pf::fail(PF_EUNSUPPORTED, "pf_gt_prepare: H*W must be below 2^31 (areas and pixel indices are 32-bit)");
    if (B > 65535) return pf::fail(PF_EUNSUPPORTED, "pf_gt_prepare: B must be at most 65535");
    const size_t isz[3] = {2, 4, 8};
    if ((uintptr_t)inst % isz[inst_kind]) return pf::fail(PF_EINVAL, "pf_gt_prepare: the map must be aligned to its element size");
    if ((((uintptr_t)ws | (uintptr_t)out_rgb | (uintptr_t)out_train | (uintptr_t)out_train_nofg) & 15) ||
        (((uintptr_t)seg_count | (uintptr_t)segs) & 3))
        return pf::fail(PF_EINVAL, "pf_gt_prepare: ws and the pixel outputs must be 16-byte aligned, seg_count and segs 4-byte aligned");
    const pf::GtLayout l = pf::gt_layout(B);
    if (ws_bytes < l.total) return pf::fail(PF_EWORKSPACE, "pf_gt_prepare: workspace %zu B < required %zu B", ws_bytes, l.total);
    hipStream_t s = (hipStream_t)stream;
    // without a list only the flags are needed
    if (int rc = pf::launch_zero_fill((char *)ws + l.flags, (segs ? l.total : l.tables) - l.flags, s)) return rc;
    pf::GtArgs a{inst, (char *)ws, l, out_rgb, out_train, out_train_nofg, seg_count, segs, (unsigned)n, B, W};
    const size_t gx = (n + pf::kGtChunkPixels - 1) / pf::kGtChunkPixels;
    const dim3 grid((unsigned)gx, (unsigned)B);
    {
        const double out_b = (out_rgb ? 3.0 : 0.0) + (out_train ? 1.0 : 0.0) + (out_train_nofg ? 1.0 : 0.0);
        pf::ProfScope ps(s, "pf::gt_stream_kernel(pf::GtArgs)", 0.0, (double)B * n * ((double)isz[inst_kind] + out_b));
        if (inst_kind == pf::kGtInstU16) hipLaunchKernelGGL((pf::gt_stream_kernel<pf::kGtInstU16>), grid, dim3(pf::kGtThreads), 0, s, a);
        else if (inst_kind == pf::kGtInstI32) hipLaunchKernelGGL((pf::gt_stream_kernel<pf::kGtInstI32>), grid, dim3(pf::kGtThreads), 0, s, a);
        else hipLaunchKernelGGL((pf::gt_stream_kernel<pf::kGtInstI64>), grid, dim3(pf::kGtThreads), 0, s, a);
        PF_LAUNCH_CHECK("gt_stream_kernel");
    }
    {
        pf::ProfScope ps(s, "pf::gt_finish_kernel(pf::GtArgs)", 0.0, (double)B * pf::kGtSlots * 4.0);
        hipLaunchKernelGGL(pf::gt_finish_kernel, dim3((unsigned)B), dim3(pf::kGtFinishThreads), 0, s, a);
        PF_LAUNCH_CHECK("gt_finish_kernel");
    }
    return PF_OK;
}

extern "C" int pf_gt_prepare_status(const void *ws, void *stream, int *host_status) {
    return pf::sticky_status_read("pf_gt_prepare_status", ws, stream, host_status);
}

extern "C" int pf_gt_prepare_status_reset(void *ws, void *stream) { return pf::sticky_status_reset("pf_gt_prepare_status_reset", ws, stream); }

extern "C" int pf_debug_gt_labels(int index, int *out8, char *name, size_t name_cap, char *category, size_t category_cap) {
    if (index < 0 || index >= pf::kGtLabelCount || !out8 || !name || !category)
        return pf::fail(PF_EINVAL, "pf_debug_gt_labels: index %d outside [0, %d) or a null output", index, pf::kGtLabelCount);
    const pf::GtLabel &l = pf::kGtLabels[index];
    const int row[8] = {l.id, l.train_id, l.category_id, l.has_instances, l.ignore_in_eval, l.r, l.g, l.b};
    for (int k = 0; k < 8; ++k) out8[k] = row[k];
    snprintf(name, name_cap, "%s", l.name);
    snprintf(category, category_cap, "%s", l.category);
    return PF_OK;
}
