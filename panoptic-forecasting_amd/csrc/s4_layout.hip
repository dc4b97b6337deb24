// fp32 NCHW <-> packed-pair ("S4") layout conversion (conv_mfma.h) and the range guard's own kernels: the check of tensors no kernel
// of this library produced, and the end-of-forward finalisation of the status words.
#include "conv_s4.h"

namespace pf {

__global__ void s4_pack_kernel(const float *src, unsigned short *dst, int B, int C, int H, int W, unsigned *status) {
    const size_t hw = (size_t)H * W, c4 = (C + 3) / 4, n = (size_t)B * c4 * hw;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t px = i % hw, g = (i / hw) % c4, b = i / (hw * c4);
        for (int r = 0; r < 4; ++r) {
            const int c = (int)g * 4 + r;
            const float x = c < C ? src[((size_t)b * C + c) * hw + px] : 0.f;
            bad = bad || !(fabsf(x) <= kSplitMaxAbs);
            split_x2 h, m;
            split_terms2(x, 0.f, h, m);
            dst[(((b * 2 + 0) * c4 + g) * hw + px) * 4 + r] = __builtin_bit_cast(unsigned short, h[0]);
            dst[(((b * 2 + 1) * c4 + g) * hw + px) * 4 + r] = __builtin_bit_cast(unsigned short, m[0]);
        }
    }
    if (bad && status) atomicOr(status, 1u);   // PF_STATUS_RANGE
}
// the range guard for tensors no kernel of this library produced (dense network inputs): overflow / NaN -> PF_STATUS_RANGE,
// max |x| -> the launch's slot (low side, conv_mfma.h)
__global__ void range_check_kernel(const float *x, size_t n, unsigned *status, unsigned *slot) {
    bool bad = false;
    float m = 0.f;
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const s4_f32x4 v = reinterpret_cast<const s4_f32x4 *>(x)[i];
        bad = bad || !(fabsf(v[0]) <= kSplitMaxAbs) || !(fabsf(v[1]) <= kSplitMaxAbs) || !(fabsf(v[2]) <= kSplitMaxAbs) ||
              !(fabsf(v[3]) <= kSplitMaxAbs);
        m = range_acc(m, v[0], v[1], v[2], v[3]);
    }
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {
        const float t = x[n4 * 4 + threadIdx.x];
        bad = bad || !(fabsf(t) <= kSplitMaxAbs);
        m = range_acc(m, t, 0.f, 0.f, 0.f);
    }
    if (bad) atomicOr(status, 1u);   // PF_STATUS_RANGE
    range_commit(status, slot, m);
}
int launch_range_check(const float *x, size_t n, unsigned *status, unsigned *slot, hipStream_t s) {
    if (!status || n == 0) return PF_OK;
    if ((reinterpret_cast<uintptr_t>(x) & 15) != 0) return fail(PF_EINVAL, "range check: input is not 16-B aligned");
    const size_t blocks = (n / 4 + 255) / 256;
    hipLaunchKernelGGL(range_check_kernel, dim3((unsigned)(blocks < 2048 ? (blocks ? blocks : 1) : 2048)), dim3(256), 0, s, x, n, status, slot);
    PF_LAUNCH_CHECK("range_check_kernel");
    return PF_OK;
}
// end of a forward: a launch whose reported maximum is below kRangeLowMax raises PF_STATUS_RANGE_LOW; the forward's status
// (the live word the kernels ORed into) is published in word 0 and ORed into the sticky word (only the host clears that one);
// the reported maxima move to the "last forward" half of the slot area, and the live word and slots are left cleared for the
// next forward (hardnet_plan.hip: no memset at the start of a forward)
__global__ void range_finalize_kernel(unsigned *st, int live_word, int first_slot, int n_slots, unsigned low_bits, int sticky_word) {
    __shared__ unsigned low;
    if (threadIdx.x == 0) low = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n_slots; i += blockDim.x) {
        const unsigned v = st[first_slot + i];
        // v = bits(max |stored value|) | 1; 0 = no report, 1 = every sampled value was exactly zero: zeros lose nothing in the
        // fp16 pair (a dead-ReLU layer, blank frames, an all-zero dense input), so only a NON-ZERO maximum below 2^-6 is low
        if ((v & ~1u) != 0 && v < low_bits) low = 1;
        st[first_slot + n_slots + i] = v;
        st[first_slot + i] = 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned w = st[live_word] | (low ? 2u : 0u);   // PF_STATUS_RANGE_LOW
        st[0] = w;
        st[sticky_word] |= w;
        st[live_word] = 0;
    }
}
int launch_range_finalize(unsigned *st, int live_word, int first_slot, int n_slots, int sticky_word, hipStream_t s) {
    hipLaunchKernelGGL(range_finalize_kernel, dim3(1), dim3(256), 0, s, st, live_word, first_slot, n_slots,
                       __builtin_bit_cast(unsigned, kRangeLowMax), sticky_word);
    PF_LAUNCH_CHECK("range_finalize_kernel");
    return PF_OK;
}
__global__ void s4_unpack_kernel(const unsigned short *src, float *dst, int B, int C, int H, int W) {
    const size_t hw = (size_t)H * W, c4 = (C + 3) / 4, n = (size_t)B * C * hw;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t px = i % hw, c = (i / hw) % C, b = i / (hw * C);
        const size_t at = ((c / 4) * hw + px) * 4 + (c & 3);
        const unsigned short h = src[(b * 2 + 0) * c4 * hw * 4 + at], m = src[(b * 2 + 1) * c4 * hw * 4 + at];
        dst[i] = (float)__builtin_bit_cast(split_t, h) + (float)__builtin_bit_cast(split_t, m);
    }
}
int launch_s4_pack(const float *src, void *dst, int B, int C, int H, int W, unsigned *status, hipStream_t s) {
    hipLaunchKernelGGL(s4_pack_kernel, dim3(1024), dim3(256), 0, s, src, (unsigned short *)dst, B, C, H, W, status);
    PF_LAUNCH_CHECK("s4_pack_kernel");
    return PF_OK;
}
int launch_s4_unpack(const void *src, float *dst, int B, int C, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(s4_unpack_kernel, dim3(1024), dim3(256), 0, s, (const unsigned short *)src, dst, B, C, H, W);
    PF_LAUNCH_CHECK("s4_unpack_kernel");
    return PF_OK;
}

}  // namespace pf
