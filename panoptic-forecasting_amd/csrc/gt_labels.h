// The public Cityscapes label table (labels.py of cityscapesScripts: 34 labels and the licence plate), the device side's one copy;
// gt_prep.LABELS is Python's, tests/test_gt_prep_host.py holds the two against each other through pf_debug_gt_labels, and against
// panoptic.TRAINID2ID (the host's copy of panoptic_ids.h's kPanTrainId2Id) and eval_common.LABEL_NAMES.  What the kernels of gt_prepare.hip read are the two tables derived
// from it at compile time: a label's trainId byte and the mask of the ignoreInEval labels.
#pragma once
#include <cstdint>

#include "panoptic_ids.h"

namespace pf {

struct GtLabel {
    const char *name;
    int id, train_id;
    const char *category;
    int category_id, has_instances, ignore_in_eval;
    int r, g, b;
};

constexpr int kGtLabelCount = 35;
constexpr GtLabel kGtLabels[kGtLabelCount] = {
    {"unlabeled", 0, 255, "void", 0, 0, 1, 0, 0, 0},
    {"ego vehicle", 1, 255, "void", 0, 0, 1, 0, 0, 0},
    {"rectification border", 2, 255, "void", 0, 0, 1, 0, 0, 0},
    {"out of roi", 3, 255, "void", 0, 0, 1, 0, 0, 0},
    {"static", 4, 255, "void", 0, 0, 1, 0, 0, 0},
    {"dynamic", 5, 255, "void", 0, 0, 1, 111, 74, 0},
    {"ground", 6, 255, "void", 0, 0, 1, 81, 0, 81},
    {"road", 7, 0, "flat", 1, 0, 0, 128, 64, 128},
    {"sidewalk", 8, 1, "flat", 1, 0, 0, 244, 35, 232},
    {"parking", 9, 255, "flat", 1, 0, 1, 250, 170, 160},
    {"rail track", 10, 255, "flat", 1, 0, 1, 230, 150, 140},
    {"building", 11, 2, "construction", 2, 0, 0, 70, 70, 70},
    {"wall", 12, 3, "construction", 2, 0, 0, 102, 102, 156},
    {"fence", 13, 4, "construction", 2, 0, 0, 190, 153, 153},
    {"guard rail", 14, 255, "construction", 2, 0, 1, 180, 165, 180},
    {"bridge", 15, 255, "construction", 2, 0, 1, 150, 100, 100},
    {"tunnel", 16, 255, "construction", 2, 0, 1, 150, 120, 90},
    {"pole", 17, 5, "object", 3, 0, 0, 153, 153, 153},
    {"polegroup", 18, 255, "object", 3, 0, 1, 153, 153, 153},
    {"traffic light", 19, 6, "object", 3, 0, 0, 250, 170, 30},
    {"traffic sign", 20, 7, "object", 3, 0, 0, 220, 220, 0},
    {"vegetation", 21, 8, "nature", 4, 0, 0, 107, 142, 35},
    {"terrain", 22, 9, "nature", 4, 0, 0, 152, 251, 152},
    {"sky", 23, 10, "sky", 5, 0, 0, 70, 130, 180},
    {"person", 24, 11, "human", 6, 1, 0, 220, 20, 60},
    {"rider", 25, 12, "human", 6, 1, 0, 255, 0, 0},
    {"car", 26, 13, "vehicle", 7, 1, 0, 0, 0, 142},
    {"truck", 27, 14, "vehicle", 7, 1, 0, 0, 0, 70},
    {"bus", 28, 15, "vehicle", 7, 1, 0, 0, 60, 100},
    {"caravan", 29, 255, "vehicle", 7, 1, 1, 0, 0, 90},
    {"trailer", 30, 255, "vehicle", 7, 1, 1, 0, 0, 110},
    {"train", 31, 16, "vehicle", 7, 1, 0, 0, 80, 100},
    {"motorcycle", 32, 17, "vehicle", 7, 1, 0, 0, 0, 230},
    {"bicycle", 33, 18, "vehicle", 7, 1, 0, 119, 11, 32},
    {"license plate", -1, -1, "vehicle", 7, 0, 1, 0, 0, 142},
};

// labelId -> trainId byte (255: none), padded to 64 entries
struct GtTrainLut {
    uint8_t t[64];
};
constexpr GtTrainLut gt_train_lut() {
    GtTrainLut l{};
    for (int i = 0; i < 64; ++i) l.t[i] = 255;
    for (int i = 0; i < kGtLabelCount; ++i)
        if (kGtLabels[i].id >= 0) l.t[kGtLabels[i].id] = (uint8_t)kGtLabels[i].train_id;
    return l;
}
constexpr GtTrainLut kGtTrainLut = gt_train_lut();

// The kernels decide everything from the trainId byte: a label is listed and coloured exactly when it has a trainId, and it is
// removed from the no-foreground map exactly when that trainId is a thing class.  The table must make that true.
constexpr bool gt_labels_consistent() {
    for (int i = 0; i < kGtLabelCount; ++i) {
        const GtLabel &l = kGtLabels[i];
        if (l.id < 0) continue;
        if (l.id != i || l.id >= kPanMaxId) return false;
        if ((l.train_id == 255) != (l.ignore_in_eval != 0)) return false;
        if ((l.has_instances && !l.ignore_in_eval) != (l.train_id >= kPanFirstThing && l.train_id < 19)) return false;
    }
    return true;
}
static_assert(gt_labels_consistent(), "ignoreInEval <=> no trainId; hasInstances and evaluated <=> trainId 11..18");

}  // namespace pf
