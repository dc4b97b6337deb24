// The scan of two label maps of different element width that conf_count_kernel and iiou_count_kernel share: typed loads, the split of
// an image into [head | units | tail], and the loop over a workgroup's chunk.  What a kernel does with the pixels is its sink.
//
// grid (pixel chunks, B): a chunk never spans two images.  Map a is the prediction (values in [0, 256)), map b the ground truth
// (values in [0, 2^BBITS)); a pixel's key is b << 8 | a.  The head (< 16 pixels) ends where both maps reach the alignment of a lane's
// load; a unit is what one lane reads per trip: P = 16 pixels where both maps are narrow (u8 / u16; the sink gets the raw 16-byte
// words), else P = 4 pixels (decoded values).  Where no head aligns both maps (u8 at +1 byte against i32 at +4) the map left
// misaligned is read by element loads in the same loop: slower, never refused.  A workgroup owns kScanChunkPixels pixels of units;
// its lanes load kScanGroup trips at once (the loads do not wait for one another) and fold runs of equal keys in registers.  The fold
// is a lane's own and ends with the workgroup, so nothing carries from image to image.  Head and tail go through per element
// (workgroup 0 of the image, one lane per pixel).  A value out of range (compared in the map's own width) makes the scan return
// false: the caller flags the image, which then adds nothing, so the trip that held the value is skipped.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace pf {

constexpr int kScanThreads = 256;             // lanes of one count workgroup
constexpr int kScanChunkPixels = 16384;       // pixels of units one count workgroup owns, whatever the kinds
constexpr int kScanGroup = 4;                 // trips whose loads are in flight together

// one element; false: a value outside [0, 2^BITS)
template <typename T, int BITS>
__device__ __forceinline__ bool load1(const T *base, size_t i, unsigned &v) {
    if (sizeof(T) * 8 <= BITS) {
        v = (unsigned)base[i];
        return true;
    }
    const unsigned long long x = (unsigned long long)(long long)base[i];   // a negative value keeps its high bits
    v = (unsigned)x;
    return (x >> BITS) == 0;
}

// four pixels from pixel i on (the generic unit); aligned: one or two vector loads, else element loads
template <typename T, int BITS>
__device__ __forceinline__ bool load4(const T *base, size_t i, bool aligned, unsigned v[4]) {
    if (!aligned) {
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) ok = load1<T, BITS>(base, i + k, v[k]) && ok;
        return ok;
    }
    if constexpr (sizeof(T) == 1) {
        const unsigned w = *reinterpret_cast<const unsigned *>(base + i);
        v[0] = w & 255u; v[1] = (w >> 8) & 255u; v[2] = (w >> 16) & 255u; v[3] = w >> 24;
        return true;
    } else if constexpr (sizeof(T) == 2) {
        const uint2 w = *reinterpret_cast<const uint2 *>(base + i);
        v[0] = w.x & 65535u; v[1] = w.x >> 16; v[2] = w.y & 65535u; v[3] = w.y >> 16;
        return true;
    } else if constexpr (sizeof(T) == 4) {
        const int4 s = *reinterpret_cast<const int4 *>(base + i);
        v[0] = (unsigned)s.x; v[1] = (unsigned)s.y; v[2] = (unsigned)s.z; v[3] = (unsigned)s.w;
        return ((v[0] | v[1] | v[2] | v[3]) >> BITS) == 0;
    } else {
        const longlong2 *s = reinterpret_cast<const longlong2 *>(base + i);
        const longlong2 s0 = s[0], s1 = s[1];
        v[0] = (unsigned)s0.x; v[1] = (unsigned)s0.y; v[2] = (unsigned)s1.x; v[3] = (unsigned)s1.y;
        return (((unsigned long long)s0.x | (unsigned long long)s0.y | (unsigned long long)s1.x | (unsigned long long)s1.y) >> BITS) == 0;
    }
}

// sixteen bytes from pixel i on as four words: sixteen u8 pixels or eight u16 pixels (every value is in range)
template <typename T>
__device__ __forceinline__ uint4 load_words(const T *base, size_t i, bool aligned) {
    static_assert(sizeof(T) <= 2, "raw words are for the narrow maps");
    if (aligned) return *reinterpret_cast<const uint4 *>(base + i);
    constexpr int E = 4 / sizeof(T);   // elements of one word
    unsigned w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        w[k] = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) w[k] |= (unsigned)base[i + E * k + e] << (8 * sizeof(T) * e);
    }
    return uint4{w[0], w[1], w[2], w[3]};
}

// bytes a lane's load of one unit of P pixels must be aligned to
template <typename T, int P> __host__ __device__ constexpr int scan_align() { return (int)(P * sizeof(T) < 16 ? P * sizeof(T) : 16); }

// an image of n pixels: head pixels [0, head), units of P pixels from there, tail pixels [tail0, n) (fewer than P)
struct ScanSpan {
    size_t head, units, tail0;
    bool al_a, al_b;   // the map is aligned for a unit's load after the head
};

// the head: the fewest pixels (below 16) after which both maps are aligned for a lane's load; failing that, map a alone
__host__ __device__ __forceinline__ ScanSpan scan_span(uintptr_t a, uintptr_t b, size_t esz_a, size_t esz_b, size_t align_a,
                                                       size_t align_b, size_t n, size_t P) {
    ScanSpan s;
    s.head = 16;
    for (int h = 15; h >= 0; --h)
        if ((a + h * esz_a) % align_a == 0 && (b + h * esz_b) % align_b == 0) s.head = h;
    if (s.head == 16)
        for (int h = 15; h >= 0; --h)
            if ((a + h * esz_a) % align_a == 0) s.head = h;
    if (s.head > n) s.head = n;
    s.al_a = (a + s.head * esz_a) % align_a == 0;
    s.al_b = (b + s.head * esz_b) % align_b == 0;
    s.units = (n - s.head) / P;
    s.tail0 = s.head + s.units * P;
    return s;
}

// a lane's run of equal keys
struct RunFold {
    unsigned cur, run;
};

template <typename Sink>
__device__ __forceinline__ void fold_pixel(RunFold &f, Sink &sink, unsigned key) {
    if (key == f.cur) {
        ++f.run;
    } else {
        if (f.run) sink.flush(f.cur, f.run);
        f.cur = key;
        f.run = 1;
    }
}

// Scans image [ab, ab + n) / [bb, bb + n) for workgroup blockIdx.x of its image; false: this lane met a value out of range.
// The sink has  flush(key, n)             a finished run of n pixels of key, and where P == 16
//               raw(fold, aw, bw)         sixteen pixels: uint4 aw of map a's bytes, uint4 bw[sizeof(BT)] of map b's; it folds them
//                                         through fold_pixel (its own caches must agree with a fold that starts at {0, 0}).
template <typename AT, typename BT, int BBITS, int P, typename Sink>
__device__ __forceinline__ bool label_scan(const AT *ab, const BT *bb, size_t n, Sink &sink) {
    constexpr bool kRaw = P == 16;
    static_assert(P == 4 || (P == 16 && sizeof(AT) == 1 && sizeof(BT) <= 2), "a unit is 4 decoded pixels or 16 raw narrow ones");
    constexpr size_t kUnitsPerChunk = kScanChunkPixels / P;
    static_assert(kUnitsPerChunk % (kScanGroup * kScanThreads) == 0, "a chunk is whole groups of trips");
    const int tid = threadIdx.x;
    const ScanSpan sp = scan_span((uintptr_t)ab, (uintptr_t)bb, sizeof(AT), sizeof(BT), scan_align<AT, P>(), scan_align<BT, P>(), n, P);
    const size_t head = sp.head;

    RunFold f{0u, 0u};
    bool ok = true;
    const size_t u0 = (size_t)blockIdx.x * kUnitsPerChunk;
    const size_t u1 = u0 + kUnitsPerChunk < sp.units ? u0 + kUnitsPerChunk : sp.units;
    for (size_t t = u0; t < u1; t += (size_t)kScanGroup * kScanThreads) {
        if constexpr (kRaw) {
            constexpr int NB = sizeof(BT);   // 16-byte loads of map b per unit
            uint4 av[kScanGroup], bv[kScanGroup][NB];
#pragma unroll
            for (int k = 0; k < kScanGroup; ++k) {
                const size_t u = t + (size_t)k * kScanThreads + tid;
                if (u < u1) {
                    av[k] = load_words(ab, head + u * P, sp.al_a);
#pragma unroll
                    for (int j = 0; j < NB; ++j) bv[k][j] = load_words(bb, head + u * P + j * (P / NB), sp.al_b);
                }
            }
#pragma unroll
            for (int k = 0; k < kScanGroup; ++k) {
                const size_t u = t + (size_t)k * kScanThreads + tid;
                if (u < u1) sink.raw(f, av[k], bv[k]);
            }
        } else {
            unsigned av[kScanGroup][4], bv[kScanGroup][4];
            bool good[kScanGroup];
#pragma unroll
            for (int k = 0; k < kScanGroup; ++k) {
                const size_t u = t + (size_t)k * kScanThreads + tid;
                good[k] = true;
                if (u < u1) {
                    const bool oka = load4<AT, 8>(ab, head + u * P, sp.al_a, av[k]);
                    const bool okb = load4<BT, BBITS>(bb, head + u * P, sp.al_b, bv[k]);
                    good[k] = oka && okb;
                }
            }
#pragma unroll
            for (int k = 0; k < kScanGroup; ++k) {
                const size_t u = t + (size_t)k * kScanThreads + tid;
                if (u >= u1) continue;
                if (!good[k]) {   // the image is flagged by the caller and adds nothing: its pixels need not be counted
                    ok = false;
                    continue;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) fold_pixel(f, sink, (bv[k][j] << 8) | av[k][j]);
            }
        }
    }
    if (f.run) sink.flush(f.cur, f.run);
    if (blockIdx.x == 0) {   // head and tail, one lane per pixel: fewer than 16 + P <= 32 of them
        const size_t ntail = n - sp.tail0;
        size_t i = n;
        if ((size_t)tid < head) i = tid;
        else if ((size_t)tid - head < ntail) i = sp.tail0 + ((size_t)tid - head);
        if (i < n) {
            unsigned a, b;
            const bool oka = load1<AT, 8>(ab, i, a), okb = load1<BT, BBITS>(bb, i, b);
            if (oka && okb) sink.flush((b << 8) | a, 1u);
            else ok = false;
        }
    }
    return ok;
}

}  // namespace pf
