// Shared by odom_net.hip (inference forward) and odom_train.hip (training forward + BPTT): the shipped shapes, the raw
// state_dict layout, the row-sum butterfly and the launch arguments of odom_forward_kernel.
#pragma once
#include "pf_common.h"

namespace pf {
namespace odom {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int H = 128;       // rnn_hidden
constexpr int G3 = 3 * H;    // gate rows r, z, n
constexpr int WAVES = 8;     // 8 x 16 units
constexpr int THREADS = WAVES * 64;
constexpr int KS = H / 4;    // k-steps of the 16x16x4 MFMA
constexpr int HP = H + 4;    // LDS row stride of h (floats)
constexpr int T_MAX = 64;    // T_in and T_out limits
constexpr int M_MAX = 3;     // 16-row sub-tiles per workgroup (M = 4 would spill: 256 VGPRs + scratch)

// the 8 state_dict tensors in the reference's order (= the raw buffer handed to pf_odom_pack)
// odom_mean [1,2], odom_std [1,2], rnn.weight_ih_l0 [384,2], rnn.weight_hh_l0 [384,128], rnn.bias_ih_l0, rnn.bias_hh_l0 [384],
// out.0.weight [2,128], out.0.bias [2]: 50 950 floats
constexpr int O_MEAN = 0, O_STD = 2, O_WIH = 4, O_WHH = O_WIH + G3 * 2, O_BIH = O_WHH + G3 * H, O_BHH = O_BIH + G3,
              O_OUTW = O_BHH + G3, O_OUTB = O_OUTW + 2 * H, RAW_TOTAL = O_OUTB + 2;
constexpr int PACKED_WHH = (RAW_TOTAL + 63) / 64 * 64;          // the re-tiled W_hh follows the raw copy
constexpr int PACKED_TOTAL = PACKED_WHH + WAVES * KS * 3 * 64;
static_assert(RAW_TOTAL == 50950, "odom state_dict size");

// one DPP butterfly over the 16 lanes of a row: every lane ends with the same sum (each stage adds a commuted pair)
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row16_sum(float v) {
    v = dpp_add<0xB1>(v);     // quad_perm [1,0,3,2]
    v = dpp_add<0x4E>(v);     // quad_perm [2,3,0,1]
    v = dpp_add<0x141>(v);    // row_half_mirror: quad 0 <-> quad 1
    v = dpp_add<0x140>(v);    // row_mirror: lanes 0-7 <-> 8-15
    return v;
}

// what the training forward keeps for the backward, per (step s, sequence b): planes of [S*B][128] (h_s, r, z, n,
// q = W_hn h + b_hn) and [S*B][2] (x_s, the step's normalised input); the backward overwrites r, z, n, q with
// da_r, da_z, da_n, dq and fills gc [S*B][2] (the gradient of a decoder step's output, 0 at encoder steps)
struct Saved {
    float *h, *r, *z, *n, *q, *x, *gc;
};

struct Args {
    const float *raw;          // raw state_dict copy inside the packed buffer
    const float *whh;          // packed W_hh
    const float *inps;         // [B][T_in][2]
    float *out, *out_norm;     // [B][T_out][2]
    int B, T_in, T_out, offset;
    Saved sv;                  // read by the SAVE instantiations only
};

int check_dims(int B, int T_in, int T_out, int flags);
int cu_count(int *cus);
// M sub-tiles per workgroup: the fewest that keep the grid at or below one workgroup per CU (at most M_MAX; past
// 16 * M_MAX * CUs sequences the grid simply grows)
static inline int pick_m(int B, int cus) {
    const long long per = 16LL * cus;
    const int m = (int)((B + per - 1) / per);
    return m < 1 ? 1 : (m > M_MAX ? M_MAX : m);
}
// odom_net.hip: odom_forward_kernel<M, true>
int launch_train_forward(const Args &a, int m, hipStream_t s);

}  // namespace odom
}  // namespace pf
