// The depth decode of the load hop, shared by hop_load_kernel (hop_kernels.hip) and bg_augment_kernel (bg_augment.hip): both
// translation units are built with -ffp-contract=off and must give the same f32 bits for the same u16 code.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace pf {

// BGDataset.__getitem__ (data/datasets/bg_dataset.py:224-228,166-170): x/256 - 1, mask = d > 0, d[~mask] = -1, clamp masked values
__device__ __forceinline__ float hop_decode(uint16_t q, float lo, float hi, uint8_t &m) {
    float d = (float)q / 256.f - 1.f;
    const bool mk = d > 0.f;
    m = mk ? 1 : 0;
    if (!mk) return -1.f;
    d = d > hi ? hi : d;    // _clamp_depths order: upper bound first, then lower (bg_dataset.py:166-170)
    d = d < lo ? lo : d;
    return d;
}

}  // namespace pf
