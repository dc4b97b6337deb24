// Device-only helpers shared by the training units (train_*.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace pf {

typedef float tr_f32x4 __attribute__((ext_vector_type(4)));

// Sums v[0..NV) over a block of 256 threads (4 waves) in a fixed order - a butterfly inside the wave, the four wave sums left to
// right through LDS - and leaves every thread with the totals.  All reductions of a training step are two-stage with fp64
// partials combined like this: a step is bit-reproducible run to run.
template <int NV>
__device__ __forceinline__ void block_reduce_d(double (&v)[NV]) {
    __shared__ double smem[NV * 4];
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) smem[k * 4 + wave] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = ((smem[k * 4 + 0] + smem[k * 4 + 1]) + smem[k * 4 + 2]) + smem[k * 4 + 3];
    __syncthreads();
}

}  // namespace pf
