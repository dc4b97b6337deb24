// Pieces shared by the packed-pair ("S4") convolution kernels: conv_s4.hip (3x3), conv_s4_1x1.hip and conv_pair.hip (an odd HarDBlock
// layer computed inside its consumer).  Layout, operand split and weight stream: conv_mfma.h, conv_s4.hip; the store rule of the layout
// (S4Dst, s4_store_px) and the finishing step in front of it (s4_finish): conv_epilogue.h.
#pragma once
#include "conv_epilogue.h"

namespace pf {

typedef float s4_f32x4 __attribute__((ext_vector_type(4)));
typedef split_x8 s4_h8;   // 8 / 4 fp16 terms (conv_mfma.h: split_terms2)
typedef split_x4 s4_h4;
typedef __attribute__((address_space(3))) void *s4_lds_ptr_t;
[[maybe_unused]] constexpr unsigned kS4Oob = 0x80000000u;

__device__ __forceinline__ s4_h8 s4_join(s4_h4 lo, s4_h4 hi) {
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// the source range that owns group entry e of the conv's K order: its tensor, groups per term, first group, groups, first entry
struct S4Owner {
    const float *sp;
    int c4, g0, gn, e0;
};
__device__ __forceinline__ S4Owner s4_owner(const ConvArgs &a, int e) {
    S4Owner r = {a.src[0], a.src_c4[0], a.src_g0[0], a.src_gn[0], 0};
#pragma unroll
    for (int k = 1; k < kConvMaxSrc; ++k) {
        const bool take = k < a.n_src && e >= a.src_ent0[k];
        r.sp = take ? a.src[k] : r.sp;
        r.c4 = take ? a.src_c4[k] : r.c4;
        r.g0 = take ? a.src_g0[k] : r.g0;
        r.gn = take ? a.src_gn[k] : r.gn;
        r.e0 = take ? a.src_ent0[k] : r.e0;
    }
    return r;
}
// group entry e (uniform: all scalar) -> (source tensor frame base, byte offset of the hi plane of its group) for a buffer resource
__device__ __forceinline__ bool s4_entry(const ConvArgs &a, int e, int b, size_t plane_bytes, const char *&base, unsigned &goff,
                                         unsigned &term_stride) {
    const S4Owner r = s4_owner(a, e);
    // entries past the groups of their range (round padding) have zero weights; the caller fetches nothing for them
    // (out-of-range pieces land as zeros), the address stays inside the tensor anyway
    base = reinterpret_cast<const char *>(r.sp) + (size_t)b * 2 * r.c4 * plane_bytes;
    goff = (unsigned)(r.g0 + min(e - r.e0, r.gn - 1)) * (unsigned)plane_bytes;
    term_stride = (unsigned)r.c4 * (unsigned)plane_bytes;
    return e - r.e0 < r.gn;
}
// its per-lane twin (the 1x1 kernel's load_round: e differs between lane groups): the hi plane as a 64-bit pointer.  (Through s4_entry's
// 32-bit offsets conv_s4_1x1_kernel<2, *> compiled to 12-16 B of scratch at its 128 registers: profiles/s4_store_unify.md)
__device__ __forceinline__ bool s4_entry_lane(const ConvArgs &a, int e, int b, size_t plane_bytes, const char *&hi, size_t &term_stride) {
    const S4Owner r = s4_owner(a, e);
    hi = reinterpret_cast<const char *>(r.sp) + ((size_t)b * 2 * r.c4 + (r.g0 + min(e - r.e0, r.gn - 1))) * plane_bytes;
    term_stride = (size_t)r.c4 * plane_bytes;
    return e - r.e0 < r.gn;
}

// weight blocks in front of round r (2 per round + one collected-tap block per started group of 4 rounds before it)
__host__ __device__ inline int s4_blocks_before(int r) { return 2 * r + r / 4; }
__host__ __device__ inline int s4_blocks_total(int rounds) { return 2 * rounds + (rounds + 3) / 4; }

// conv_s4_1x1.hip: the 1x1 kernel with NT cout tiles per workgroup, EPI = 1 with the fused epilogue stages (pool, residual, no bias);
// instantiated there for NT = 1 .. 4
template <int NT, int EPI>
int launch_s41_cfg(const ConvArgs &a, int B, hipStream_t s);

}  // namespace pf
