// The op table of a weight blob (pf_blob.h), as the inference plan (plan_create.hip) and the training plan (train_plan.hip)
// both hold it: parsed and checked once, and the spatial size of every tensor for a given network input.
#pragma once
#include <cstddef>
#include <vector>

#include "pf_blob.h"

namespace pf {

struct NetTable {
    BlobHeader hdr;
    std::vector<BlobTensor> tensors;
    std::vector<BlobOp> ops;
};

// header (magic, version, table offsets, in_ch / n_cls) and, per op, source count, tensor indices and channel ranges.  What
// only one kind of plan requires (weight offsets, the supported convolutions) is checked by that plan.  On a per-op failure the
// tables stay filled in (the caller may still rank a limit of its own above it)
int parse_net_table(const void *blob, size_t bytes, int in_ch, int n_cls, NetTable &t);

struct Dims {
    int h = 0, w = 0;
};

// spatial size of every tensor for an H x W network input
int propagate_dims(const NetTable &t, int H, int W, std::vector<Dims> &d);

}  // namespace pf
