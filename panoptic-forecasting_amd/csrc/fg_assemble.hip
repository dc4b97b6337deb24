// Batch assembly of the fg export path on the device - restates, for all scenes of a batch at once, what
// FGSceneDataset.__getitem__ computes per scene once the host has selected the has_gt rows and the bbox_inds columns
// (data/datasets/fg_scene_dataset.py:380-454): box conversion, the car-gap filter (:300-340), velocities, depth masks and depth
// velocities, class offsets / one-hot, and the gather of the [256,14,14] feature planes.  Outputs are in the concatenated [N, ...]
// layout FGModel._predict builds with torch.cat.
//
// Exactness: the reference calls .float() and then does its arithmetic in fp32, one operation per step ((a + b) / 2, a - b,
// a + gap, (a - b) * {0,1} and comparisons); the kernel does the same single fp32 operations in the same order (built with FP
// contraction off), so every output is bit-identical to torch's.  The quirk of _filter_car_gap is kept: it reads x0, y0, x1, y1
// from the boxes AFTER the cwh conversion, so without use_ulbr it compares cx and w.
//
//   grid  : one launch, 1-D.  Blocks [0, N * T_in * FGA_SPLIT): block = (plane n * T_in + t, piece) copies 1/FGA_SPLIT of one
//           200 704-byte plane - 1792 16-byte pieces, 7 per lane, all 7 loads issued before the first store; N = 1 is 21 blocks.
//           Blocks after those: one lane per instance, the T steps and the scan in registers.
//   guard : feat_row outside [0, M) is never followed as an address: the plane is written as zeros.
//   bytes : 2 * N * T_in * 200 704 for the gather; the per-instance part moves 462 bytes per instance.
#include "pf_common.h"
#include "pf_prof.h"

namespace pf {

typedef float fga_f4 __attribute__((ext_vector_type(4)));

constexpr int FGA_T = 6;                          // steps per instance (3 inputs + 3 outputs: the only shape the dataset yields)
constexpr int FGA_THREADS = 256;
constexpr int FGA_PLANE4 = 256 * 14 * 14 / 4;     // 12 544 16-byte pieces per plane
constexpr int FGA_SPLIT = 7;                      // workgroups per plane
constexpr int FGA_PER_LANE = FGA_PLANE4 / FGA_SPLIT / FGA_THREADS;   // 7
static_assert(FGA_SPLIT * FGA_THREADS * FGA_PER_LANE == FGA_PLANE4, "a plane splits evenly");
constexpr int FGA_CAR = 13;                       // trainId the car-gap filter acts on
constexpr int FGA_FIRST_THING = 11;
constexpr int FGA_THINGS = 8;

struct FgAsmArgs {
    const float *bboxes;        // [N][T][4] ulbr
    const uint8_t *feat_mask;   // [N][T]
    const float *depth;         // [N][T]
    const int *classes;         // [N] trainIds
    const int *feat_row;        // [N][T_in]
    const fga_f4 *feat_table;   // [M] planes
    float *traj;                // [N][T][8]
    uint8_t *bbox_masks, *vel_masks, *feat_masks;   // [N][T]
    float *depths;              // [N][T][2]
    uint8_t *depth_masks;       // [N][T]
    long long *classes_out;     // [N]
    float *one_hot;             // [N][8]
    float *final_bboxes;        // [N][4]
    fga_f4 *feats;              // [N][T_in] planes
    int N, T_in, M, gather_blocks;
    int use_ulbr, has_max_depth, has_gap;
    float max_depth, gap, gap_hi;                   // gap_hi = float(img_w - gap)
};

__device__ __forceinline__ void fga_gather(const FgAsmArgs &a) {
    const int plane = blockIdx.x / FGA_SPLIT, piece = blockIdx.x - plane * FGA_SPLIT;
    const int row = a.feat_row[plane];
    const size_t off = (size_t)piece * (FGA_THREADS * FGA_PER_LANE) + threadIdx.x;
    fga_f4 *dst = a.feats + (size_t)plane * FGA_PLANE4 + off;
    fga_f4 v[FGA_PER_LANE];
    if ((unsigned)row < (unsigned)a.M) {
        const fga_f4 *src = a.feat_table + (size_t)row * FGA_PLANE4 + off;
#pragma unroll
        for (int j = 0; j < FGA_PER_LANE; ++j) v[j] = src[j * FGA_THREADS];
    } else {
#pragma unroll
        for (int j = 0; j < FGA_PER_LANE; ++j) v[j] = fga_f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < FGA_PER_LANE; ++j) dst[j * FGA_THREADS] = v[j];
}

__device__ __forceinline__ void fga_instance(const FgAsmArgs &a, int n) {
    float box[FGA_T][4], d[FGA_T];
    bool bm[FGA_T], fm[FGA_T], dm[FGA_T];
    const int cls = a.classes[n];
#pragma unroll
    for (int t = 0; t < FGA_T; ++t) {
        const fga_f4 b = *reinterpret_cast<const fga_f4 *>(a.bboxes + ((size_t)n * FGA_T + t) * 4);
        if (a.use_ulbr) {
            box[t][0] = b[0], box[t][1] = b[1], box[t][2] = b[2], box[t][3] = b[3];
        } else {                                                  // convert_bbox_ulbr_cwh
            box[t][0] = (b[0] + b[2]) / 2.f;
            box[t][1] = (b[1] + b[3]) / 2.f;
            box[t][2] = b[2] - b[0];
            box[t][3] = b[3] - b[1];
        }
        bm[t] = fm[t] = a.feat_mask[(size_t)n * FGA_T + t] != 0;
        d[t] = a.depth[(size_t)n * FGA_T + t];
        dm[t] = d[t] != -1.f && d[t] != 1000000.f && (!a.has_max_depth || d[t] <= a.max_depth);
    }
    if (a.has_gap && cls == FGA_CAR) {                            // _filter_car_gap: a sequential scan over the steps
        bool have_past = false, found_x0 = false, found_x1 = false, zero_rest = false;
        float past = 0.f;
#pragma unroll
        for (int t = 0; t < FGA_T; ++t) {
            if (!zero_rest) {
                if (!bm[t]) continue;
                const float x0 = box[t][0], x1 = box[t][2];
                if (x0 < a.gap) found_x0 = true;
                if (x1 > a.gap_hi) found_x1 = true;
                if (found_x0) {
                    if (!have_past) have_past = true;
                    else if (x1 > past + a.gap) zero_rest = true;
                    past = x1;
                }
                if (found_x1) {
                    if (!have_past) have_past = true;
                    else if (x0 < past - a.gap) zero_rest = true;
                    past = x0;
                }
            }
            if (zero_rest) {
                bm[t] = fm[t] = false;
                box[t][0] = box[t][1] = box[t][2] = box[t][3] = 0.f;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < FGA_T; ++t) {
        const size_t i = (size_t)n * FGA_T + t;
        const bool pair = t > 0 && bm[t] && bm[t - 1];
        const bool dpair = t > 0 && dm[t] && dm[t - 1];
        fga_f4 vel = {0.f, 0.f, 0.f, 0.f};
        float dvel = 0.f;
        if (t > 0) {                                              // difference TIMES the 0/1 mask, as the reference multiplies
            const float m = pair ? 1.f : 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) vel[k] = (box[t][k] - box[t - 1][k]) * m;
            dvel = (d[t] - d[t - 1]) * (dpair ? 1.f : 0.f);
        }
        fga_f4 *tr = reinterpret_cast<fga_f4 *>(a.traj + i * 8);
        tr[0] = fga_f4{box[t][0], box[t][1], box[t][2], box[t][3]};
        tr[1] = vel;
        a.bbox_masks[i] = bm[t];
        a.vel_masks[i] = pair;
        a.feat_masks[i] = fm[t];
        a.depths[i * 2] = d[t];
        a.depths[i * 2 + 1] = dvel;
        a.depth_masks[i] = dm[t];
    }
    const int c = cls - FGA_FIRST_THING;
    a.classes_out[n] = c;
    fga_f4 *oh = reinterpret_cast<fga_f4 *>(a.one_hot + (size_t)n * FGA_THINGS);
    oh[0] = fga_f4{c == 0 ? 1.f : 0.f, c == 1 ? 1.f : 0.f, c == 2 ? 1.f : 0.f, c == 3 ? 1.f : 0.f};
    oh[1] = fga_f4{c == 4 ? 1.f : 0.f, c == 5 ? 1.f : 0.f, c == 6 ? 1.f : 0.f, c == 7 ? 1.f : 0.f};
    *reinterpret_cast<fga_f4 *>(a.final_bboxes + (size_t)n * 4) =
        fga_f4{box[FGA_T - 1][0], box[FGA_T - 1][1], box[FGA_T - 1][2], box[FGA_T - 1][3]};
}

__global__ __launch_bounds__(FGA_THREADS) void fg_assemble_kernel(FgAsmArgs a) {
    if ((int)blockIdx.x < a.gather_blocks) {
        fga_gather(a);
    } else {
        const int n = ((int)blockIdx.x - a.gather_blocks) * FGA_THREADS + threadIdx.x;
        if (n < a.N) fga_instance(a, n);
    }
}

}  // namespace pf

extern "C" int pf_fg_assemble(const float *bboxes, const uint8_t *feat_mask, const float *depth, const int32_t *classes,
                              const int32_t *feat_row, const float *feat_table, int N, int T, int T_in, int M, int use_ulbr,
                              double max_depth, double filter_car_gap, int img_w, float *trajectories, uint8_t *bbox_masks,
                              uint8_t *bbox_vel_masks, uint8_t *feat_masks, float *depths, uint8_t *depth_masks, int64_t *classes_out,
                              float *one_hot_classes, float *final_bboxes, float *feats, void *stream) {
    if (N < 0 || M < 0 || T_in < 0 || T_in > T) return pf::fail(PF_EINVAL, "pf_fg_assemble: bad dims N=%d T=%d T_in=%d M=%d", N, T, T_in, M);
    if (T != pf::FGA_T) return pf::fail(PF_EUNSUPPORTED, "pf_fg_assemble: T = %d steps (%d are built)", T, pf::FGA_T);
    if (N == 0) return PF_OK;
    if (!bboxes || !feat_mask || !depth || !classes || !trajectories || !bbox_masks || !bbox_vel_masks || !feat_masks || !depths ||
        !depth_masks || !classes_out || !one_hot_classes || !final_bboxes)
        return pf::fail(PF_EINVAL, "pf_fg_assemble: null table or output pointer");
    if (T_in > 0 && (!feat_row || !feats)) return pf::fail(PF_EINVAL, "pf_fg_assemble: T_in > 0 needs feat_row and feats");
    if (M > 0 && !feat_table) return pf::fail(PF_EINVAL, "pf_fg_assemble: M > 0 needs feat_table");
    if (((uintptr_t)bboxes | (uintptr_t)feat_table | (uintptr_t)trajectories | (uintptr_t)one_hot_classes | (uintptr_t)final_bboxes |
         (uintptr_t)feats) & 15)
        return pf::fail(PF_EINVAL, "pf_fg_assemble: bboxes, feat_table, trajectories, one_hot_classes, final_bboxes and feats must be 16-byte aligned");
    if (((uintptr_t)depth | (uintptr_t)classes | (uintptr_t)feat_row | (uintptr_t)depths) & 3 || ((uintptr_t)classes_out & 7))
        return pf::fail(PF_EINVAL, "pf_fg_assemble: depth, classes, feat_row, depths must be 4-byte and classes_out 8-byte aligned");
    const long long gather_blocks = (long long)N * T_in * pf::FGA_SPLIT;
    const long long blocks = gather_blocks + (N + pf::FGA_THREADS - 1) / pf::FGA_THREADS;
    if (blocks > 0x7fffffffLL) return pf::fail(PF_EUNSUPPORTED, "pf_fg_assemble: N * T_in too large for one launch");
    pf::FgAsmArgs a{};
    a.bboxes = bboxes, a.feat_mask = feat_mask, a.depth = depth, a.classes = classes, a.feat_row = feat_row;
    a.feat_table = reinterpret_cast<const pf::fga_f4 *>(feat_table);
    a.traj = trajectories, a.bbox_masks = bbox_masks, a.vel_masks = bbox_vel_masks, a.feat_masks = feat_masks, a.depths = depths;
    a.depth_masks = depth_masks, a.classes_out = reinterpret_cast<long long *>(classes_out), a.one_hot = one_hot_classes;
    a.final_bboxes = final_bboxes, a.feats = reinterpret_cast<pf::fga_f4 *>(feats);
    a.N = N, a.T_in = T_in, a.M = M, a.gather_blocks = (int)gather_blocks;
    a.use_ulbr = use_ulbr != 0, a.has_max_depth = max_depth >= 0, a.has_gap = filter_car_gap >= 0;
    // torch compares and adds a Python number with a float32 tensor in float32: the number is rounded once, and
    // img_size[0] - filter_car_gap is Python arithmetic (double) rounded once
    a.max_depth = (float)max_depth, a.gap = (float)filter_car_gap, a.gap_hi = (float)((double)img_w - filter_car_gap);
    hipStream_t s = (hipStream_t)stream;
    const double bytes = 2.0 * N * T_in * pf::FGA_PLANE4 * 16.0 + 462.0 * N;
    pf::ProfScope ps(s, "pf::fg_assemble_kernel(pf::FgAsmArgs)", 0.0, bytes);
    hipLaunchKernelGGL(pf::fg_assemble_kernel, dim3((unsigned)blocks), dim3(pf::FGA_THREADS), 0, s, a);
    PF_LAUNCH_CHECK("fg_assemble_kernel");
    return PF_OK;
}
