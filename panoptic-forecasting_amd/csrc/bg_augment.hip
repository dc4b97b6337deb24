// Training-time augmentation of BGDataset on the device (DESIGN.md "bg_augment") - replaces, per batch, what the reference does per
// sample in PIL / OpenCV on its loader workers (data/transforms.py:183-293: joint random scale / pad / crop / nearest resize / flip
// of T label maps, 1 ground-truth map and T depth planes) and the depth decode that follows (bg_dataset.py:224-228).
//
// Every step of that transform acts on one axis, so the whole of it is four index tables per sample, built on the host
// (bg_augment.py: the rounding rules of PIL and OpenCV differ, the tables carry them and the flip):
//     out[y][x] = src[y_tab[y]][x_tab[x]]      or the padding value where either entry lies outside the source.
// The kernel is that gather.  A table entry is never followed as an address unless 0 <= entry < extent.
//
//   grid  : one workgroup per (sample, block of BGA_ROWS output rows), 1-D
//   LDS   : the sample's two x tables (2 * ow ints), entries outside [0, Ws) stored as -1
//   lane  : 4 consecutive output pixels of one row, all T + 1 u8 planes and all T depth planes from the same four indices;
//           with ow % 4 == 0 and aligned bases one 4-B store per u8 plane, one 16-B store of depth and one 4-B store of mask per
//           depth plane; scalar stores otherwise (ragged last quad included)
// Reads are element-granular gathers (1 or 2 B): along x they are monotone with stride crop/size (or reversed), so a wave's 256
// pixels touch a contiguous span of about 256 * crop/size source bytes per plane - the caches serve it; all offsets are 64-bit.
#include "hop_decode.h"
#include "pf_common.h"
#include "pf_prof.h"

namespace pf {

typedef float bga_f4 __attribute__((ext_vector_type(4)));

constexpr int BGA_ROWS = 8;
constexpr int BGA_THREADS = 256;
constexpr int BGA_MAX_OW = 8192;      // 2 tables * 8192 * 4 B = 64 KiB of LDS

struct BgAugArgs {
    const uint8_t *seg_src;     // [B][T][Hs][Ws]
    const uint8_t *label_src;   // [B][Hs][Ws] (nullable)
    const uint16_t *depth_src;  // [B][T][Hs][Ws] (nullable)
    const int *y_map, *x_map;   // [B][oh], [B][ow]  label maps
    const int *y_arr, *x_arr;   // [B][oh], [B][ow]  depth arrays
    uint8_t *out_seg;           // [B][T][oh][ow]
    uint8_t *out_label;         // [B][oh][ow]
    float *out_depth;           // [B][T][oh][ow]
    uint8_t *out_mask;          // [B][T][oh][ow]
    int T, Hs, Ws, oh, ow, row_blocks;
    int pad_label, vec;
    float min_depth, max_depth;
};

// four pixels of one u8 plane: src is the plane's source ROW (nullptr: the row is padding), xi the four column indices (-1: padding)
__device__ __forceinline__ void bga_u8_quad(const uint8_t *src, const int (&xi)[4], uint8_t pad, uint8_t *dst, int nvalid, bool vec) {
    uint8_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (src && xi[j] >= 0) ? src[xi[j]] : pad;
    if (vec) {
        *reinterpret_cast<uchar4 *>(dst) = make_uchar4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nvalid) dst[j] = v[j];
    }
}

__global__ __launch_bounds__(BGA_THREADS) void bg_augment_kernel(BgAugArgs a) {
    extern __shared__ __attribute__((aligned(16))) int bga_lds[];
    int *xm = bga_lds, *xa = bga_lds + a.ow;
    const int b = blockIdx.x / a.row_blocks;
    const int row0 = (blockIdx.x - b * a.row_blocks) * BGA_ROWS;
    for (int i = threadIdx.x; i < a.ow; i += BGA_THREADS) {
        const int m = a.x_map[(size_t)b * a.ow + i];
        xm[i] = (unsigned)m < (unsigned)a.Ws ? m : -1;
        if (a.depth_src) {
            const int r = a.x_arr[(size_t)b * a.ow + i];
            xa[i] = (unsigned)r < (unsigned)a.Ws ? r : -1;
        }
    }
    __syncthreads();
    const int quads = (a.ow + 3) >> 2;
    const size_t src_plane = (size_t)a.Hs * a.Ws, out_plane = (size_t)a.oh * a.ow;
    const uint8_t pad = (uint8_t)a.pad_label;
    for (int item = threadIdx.x; item < BGA_ROWS * quads; item += BGA_THREADS) {
        const int r = item / quads, x0 = (item - r * quads) << 2;
        const int oy = row0 + r;
        if (oy >= a.oh) break;          // items are row-major: every later item of this lane lies below the image too
        const int nvalid = a.ow - x0 < 4 ? a.ow - x0 : 4;
        const size_t out_off = (size_t)oy * a.ow + x0;
        int xi[4];
        {   // label maps: T seg planes + the ground-truth plane share (ym, xm)
            const int ym = a.y_map[(size_t)b * a.oh + oy];
            const bool row_ok = (unsigned)ym < (unsigned)a.Hs;
#pragma unroll
            for (int j = 0; j < 4; ++j) xi[j] = j < nvalid ? xm[x0 + j] : -1;
            for (int t = 0; t < a.T; ++t) {
                const size_t p = (size_t)b * a.T + t;
                const uint8_t *row = row_ok ? a.seg_src + p * src_plane + (size_t)ym * a.Ws : nullptr;
                bga_u8_quad(row, xi, pad, a.out_seg + p * out_plane + out_off, nvalid, a.vec);
            }
            if (a.label_src) {
                const uint8_t *row = row_ok ? a.label_src + (size_t)b * src_plane + (size_t)ym * a.Ws : nullptr;
                bga_u8_quad(row, xi, pad, a.out_label + (size_t)b * out_plane + out_off, nvalid, a.vec);
            }
        }
        if (a.depth_src) {
            const int ya = a.y_arr[(size_t)b * a.oh + oy];
            const bool row_ok = (unsigned)ya < (unsigned)a.Hs;
#pragma unroll
            for (int j = 0; j < 4; ++j) xi[j] = j < nvalid ? xa[x0 + j] : -1;
            for (int t = 0; t < a.T; ++t) {
                const size_t p = (size_t)b * a.T + t;
                const uint16_t *row = a.depth_src + p * src_plane + (size_t)(row_ok ? ya : 0) * a.Ws;
                bga_f4 d;
                uint8_t m[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint16_t q = (row_ok && xi[j] >= 0) ? row[xi[j]] : (uint16_t)0;   // np.pad(constant_values=0): code 0
                    d[j] = hop_decode(q, a.min_depth, a.max_depth, m[j]);
                }
                float *od = a.out_depth + p * out_plane + out_off;
                uint8_t *om = a.out_mask + p * out_plane + out_off;
                if (a.vec) {
                    *reinterpret_cast<bga_f4 *>(od) = d;
                    *reinterpret_cast<uchar4 *>(om) = make_uchar4(m[0], m[1], m[2], m[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < nvalid) {
                            od[j] = d[j];
                            om[j] = m[j];
                        }
                }
            }
        }
    }
}

}  // namespace pf

extern "C" int pf_bg_augment(const uint8_t *seg_src, const uint8_t *label_src, const uint16_t *depth_src, int B, int T, int Hs, int Ws,
                             const int *y_map, const int *x_map, const int *y_arr, const int *x_arr, int oh, int ow, int pad_label,
                             float min_depth, float max_depth, uint8_t *out_seg, uint8_t *out_label, float *out_depth,
                             uint8_t *out_mask, void *stream) {
    if (B < 0 || T < 1 || Hs < 1 || Ws < 1 || oh < 1 || ow < 1)
        return pf::fail(PF_EINVAL, "pf_bg_augment: bad dims B=%d T=%d Hs=%d Ws=%d oh=%d ow=%d", B, T, Hs, Ws, oh, ow);
    if (pad_label < 0 || pad_label > 255) return pf::fail(PF_EINVAL, "pf_bg_augment: pad_label must fit a byte, got %d", pad_label);
    if (ow > pf::BGA_MAX_OW) return pf::fail(PF_EUNSUPPORTED, "pf_bg_augment: ow = %d exceeds %d (x tables live in LDS)", ow, pf::BGA_MAX_OW);
    if (B == 0) return PF_OK;
    if (!seg_src || !out_seg || !y_map || !x_map) return pf::fail(PF_EINVAL, "pf_bg_augment: null seg / label-map table pointer");
    if (label_src && !out_label) return pf::fail(PF_EINVAL, "pf_bg_augment: label_src needs out_label");
    if (depth_src && (!out_depth || !out_mask || !y_arr || !x_arr))
        return pf::fail(PF_EINVAL, "pf_bg_augment: depth_src needs out_depth, out_mask and the two array tables");
    if ((uintptr_t)depth_src & 1) return pf::fail(PF_EINVAL, "pf_bg_augment: depth_src must be 2-byte aligned");
    if (((uintptr_t)y_map | (uintptr_t)x_map | (uintptr_t)y_arr | (uintptr_t)x_arr | (uintptr_t)out_depth) & 3)
        return pf::fail(PF_EINVAL, "pf_bg_augment: tables and out_depth must be 4-byte aligned");
    const int row_blocks = (oh + pf::BGA_ROWS - 1) / pf::BGA_ROWS;
    if ((long long)row_blocks * B > 0x7fffffffLL) return pf::fail(PF_EUNSUPPORTED, "pf_bg_augment: B * oh too large for one launch");
    const bool vec = (ow & 3) == 0 && (((uintptr_t)out_depth & 15) == 0) &&
                     ((((uintptr_t)out_seg | (uintptr_t)out_label | (uintptr_t)out_mask) & 3) == 0);
    pf::BgAugArgs a{seg_src, label_src, depth_src, y_map, x_map, y_arr, x_arr, out_seg, out_label, out_depth, out_mask,
                    T, Hs, Ws, oh, ow, row_blocks, pad_label, vec ? 1 : 0, min_depth, max_depth};
    hipStream_t s = (hipStream_t)stream;
    const double px = (double)B * oh * ow;
    const double bytes = px * ((T + (label_src ? 1 : 0)) * 2.0 + (depth_src ? T * 7.0 : 0.0)) + 4.0 * B * (2.0 * oh + 2.0 * ow);
    pf::ProfScope ps(s, "pf::bg_augment_kernel(pf::BgAugArgs)", 0.0, bytes);
    hipLaunchKernelGGL(pf::bg_augment_kernel, dim3(row_blocks * B), dim3(pf::BGA_THREADS), 2 * (size_t)ow * sizeof(int), s, a);
    PF_LAUNCH_CHECK("bg_augment_kernel");
    return PF_OK;
}
