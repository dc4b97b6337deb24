// The Cityscapes id of each of the 19 trainIds (labels.py's trainId2label), the one table behind the panoptic export's
// id conversion (panoptic_merge.hip) and the panoptic-quality kernels' reading of exported ids (pq_kernels.hip).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace pf {

static __constant__ const uint8_t kPanTrainId2Id[19] = {7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33};
constexpr int kPanMaxId = 34;        // every Cityscapes id is below this
constexpr int kPanFirstThing = 11;   // trainIds 11..18 are the thing classes

}  // namespace pf
