// fg forecaster network (FGModel.forward, models/fg/fg_model.py:216-339, shipped config) on gfx950: what its units share.
//   fg_schedule.cpp  host only: tensor / GEMM tables, weight and workspace layouts, build_fg_schedule - every launch of a forward
//                    and its buffers, decided before anything is enqueued - and pf_debug_fg_schedule, which hands it to tests
//   fg_pack.hip      pf_fg_pack and its kernels          fg_gemm.hip   the two matrix cores and the status kernel
//   fg_traj.hip      the small VALU kernels              fg_net.hip    pf_fg_forward: resolves regions to pointers, enqueues the steps
// Every launch is a kernel node (no memset, no memcpy): a pf_fg_forward call can be captured into a graph.
#pragma once
#include <vector>

#include "conv_mfma.h"
#include "pf_common.h"

namespace pf {
namespace fg {

constexpr int HW = 196;      // 14 x 14
constexpr int C = 256;       // mask feature / hidden channels
constexpr int HID = 128;     // GRU hidden size
constexpr int TR = 10;       // trajectory values: 8 box + 2 depth
constexpr int OD = 5;        // odometry values
constexpr int TF = 16;       // traj_feat_channels
constexpr int IFH = 64;      // instance_feat_hidden
constexpr int ICC = 8;       // instance_feat_channels

// the 52 state_dict tensors, in the reference's state_dict order (= the order of the raw buffer handed to pf_fg_pack); a GEMM's bias
// follows its weight
enum {
    ODOM_MEAN, ODOM_STD, DEPTH_MEAN, DEPTH_STD, TRAJ_MEAN, TRAJ_STD,
    TE_WIH, TE_WHH, TE_BIH, TE_BHH, TD_WIH, TD_WHH, TD_BIH, TD_BHH,
    TEO_W0, TEO_B0, TEO_W2, TEO_B2, TDO_W0, TDO_B0, TDO_W2, TDO_B2, TFO_W, TFO_B,
    IC_W, IC_B, IF_W, IF_B,
    ME0_W, ME0_B, ME1_W, ME1_B, MD0_W, MD0_B, MD1_W, MD1_B,
    MEO_W, MEO_B, MDO_W, MDO_B,
    F1_W, F1_B, F2_W, F2_B, F3_W, F3_B, F4_W, F4_B, DC_W, DC_B, PR_W, PR_B, NTENSOR
};
extern const long long kSize[NTENSOR];

// GEMMs whose weights are packed [tile][K][64] behind the raw copy
enum { G_ME0, G_ME1, G_MD0, G_MD1, G_MEO, G_MDO, G_F1, G_F2, G_F3, G_F4, G_DC, NGEMM };
enum { MAP_LSTM = 0, MAP_PLAIN = 1, MAP_KMAJOR = 2 };
struct GemmDesc {
    int src, ctot, taps, tiles, map;
};
extern const GemmDesc kGemm[NGEMM];

struct Layout {
    size_t raw[NTENSOR], raw_total, gemm[NGEMM], total;
};
Layout layout();

// PF_FG_PAIR: behind the flags = 0 layout (kept whole: the 1x1 GEMMs and the deconvolution read it) a pair section,
//   [0 .. 7]  max |w| of the eight 3x3 GEMMs (bit patterns)   [8 .. 15]  their 2^-k   (64 floats)
//   then per 3x3 GEMM [tile][round of 16 channels][term hi, mid][tap][64 columns][16 channels] fp16 of w * 2^k, zero past ctot
constexpr int PKC = 16;                            // channels per round of pair_kernel
constexpr int PTERM_X = 256 * PKC;                 // fp16 per term of its activation planes in LDS
constexpr int PTERM_W = 9 * 64 * PKC;              // fp16 per term of a round's weights
constexpr int PROUND = 2 * PTERM_W;                // fp16 per (tile, round) of the packed pair weights
constexpr int NPAIR = 8;
extern const int kPairGemm[NPAIR];
struct PairLayout {
    size_t head, gemm[NPAIR], total;    // floats from the start of the packed buffer
};
PairLayout pair_layout(const Layout &L);

constexpr int FG_STATUS_WORDS = 256;               // status block at the head of a PF_FG_PAIR workspace
constexpr int FG_SLOT0 = 8;                        // its words 8 ..: max |v| bit patterns, three (vec, x, h) per pair launch

// ------------------------------------------------------------------------------------------------------ kernel arguments
enum { EPI_LSTM = 0, EPI_RELU = 1, EPI_BIAS = 2, EPI_DECONV = 3 };

struct GemmArgs {
    const float *vec;           // [n*vec_stride + c], c < nvec
    long long vec_stride;
    int nvec;
    const float *x;             // [n*x_stride + c*196 + p], c < nx
    long long x_stride;
    int nx;
    const float *h;             // [n*h_stride + c*196 + p], c < nh; nullptr: zero state (K half skipped, c_prev = 0)
    long long h_stride;
    int nh;
    int ctot;                   // channels of the packed K (nvec + nx + nh)
    const float *w;             // packed [tiles][ctot*TAPS][64]
    const float *bias;
    float *out;                 // EPI_LSTM: h' [n*out_stride + j*196 + p]; EPI_DECONV: [n*out_stride + co*784 + 28y' + x']
    long long out_stride;
    float *c;                   // EPI_LSTM: cell state [n][256][196], updated in place
};

struct PairArgs {
    GemmArgs g;                 // g.w unused
    const split_t *wp;          // [tile][round][term][tap][64][16] fp16 terms of w * 2^k, zero past ctot
    const float *scale;         // 2^-k (device: k is found on the device at pack time)
    unsigned *status;           // word 0 of the status block
    unsigned *slots;            // this launch's three slots
};

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }

struct TrajArgs {
    const float *trajs, *traj_mask, *vel_mask, *depths, *depth_mask, *odom;
    int T_in, T_out, odom_T;
    const float *instf;         // [N][T_in][64] (encoder) / [N][64] (decoder)
    float *gru_h;               // [N][128]
    float *tfeat;               // [N][T_in][16] (encoder) / [N][16] (decoder)
    float *traj_norm, *traj_unnorm;     // [N][1+T_out][10]
    int step;                   // decoder step
    // resolved raw offsets
    const float *odom_mean, *odom_std, *depth_mean, *depth_std, *traj_mean, *traj_std;
    const float *wih, *whh, *bih, *bhh, *w0, *b0, *w2, *b2, *wtf, *btf;
};

// -------------------------------------------------------------------------------------------------------------- schedule
// what a step's operand lives in: a region of the workspace (floats, 64-float aligned, in this order behind the status block) or one of
// the caller's tensors
enum Region {
    R_NONE, R_STATUS, R_INSTF, R_INSTD, R_GRUH, R_TFE, R_TFD, R_H0, R_C0, R_H1, R_C1, R_YA, R_YB, R_YD,
    R_FEATS, R_MASK_FEATS, R_OUTPUT_FEATS, R_MASKS, NREGION
};
struct Ws {
    size_t off[R_FEATS], floats[R_FEATS];      // of the workspace regions, from the workspace's start (behind R_STATUS: PF_FG_PAIR only)
    size_t total;                              // bytes
    int r0;                                    // slots of the h0 ring
};
Ws ws_layout(int N, int T_in, int flags);
int check_dims(int N, int T_in, int T_out, int flags, int known = PF_FG_PAIR);

enum StepKind { K_STATUS, K_INST_FEAT, K_TRAJ_ENC, K_TRAJ_DEC, K_GEMM, K_PAIR, K_GATHER, K_PREDICT };
struct Operand {
    int region;                 // R_NONE: the launch has no such operand
    long long off, stride;      // floats: from the region's start, from one instance to the next
};
// one launch with everything the enqueue loop needs.  K_GEMM / K_PAIR: the operands of GemmArgs.  K_INST_FEAT: x -> out.  K_TRAJ_*: x =
// instance features, out = traj_feat_out, c = the GRU state.  K_GATHER, K_PREDICT: x -> out
struct Step {
    int kind;
    int gemm, epi;              // K_GEMM / K_PAIR: which of kGemm (weights, bias, taps, column tiles) and its epilogue
    int nvec, nx, nh;           // channels of the three K sources (nh also when h is absent: the first cell of a layer)
    Operand vec, x, h, out, c;
    int pair, slot;             // K_PAIR: which of kPairGemm (weight section, scale) and of the launch slots of the status block
    int t;                      // K_INST_FEAT / K_TRAJ_*: the decoder step, -1 = the encoder's launch over all T_in steps
    const char *label;          // of the ProfScope
};
// the whole forward in launch order; nothing is enqueued.  Fails (PF_EINVAL) when PF_FG_PAIR is asked for a 3x3 GEMM without a pair form
int build_fg_schedule(int N, int T_in, int T_out, int flags, std::vector<Step> &steps);

// ------------------------------------------------------------------------------------------------------------- launchers
int launch_status(unsigned *st, int begin, hipStream_t s);                                                          // fg_gemm.hip
int launch_gemm(const GemmArgs &a, int taps, int epi, int N, int tiles, const char *label, hipStream_t s);
int launch_pair(const PairArgs &a, int epi, int N, int tiles, const char *label, hipStream_t s);
int launch_inst_feat(const float *x, long long x_stride, long long t_stride, const float *mask, int N, int T, const float *raw,     // fg_traj.hip
                     const Layout &L, float *out, const char *label, hipStream_t s);
int launch_traj(const TrajArgs &a, bool decoder, int N, const char *label, hipStream_t s);
int launch_gather(const float *mask_feats, const int64_t *sel, int N, int T_out, float *out, hipStream_t s);
int launch_predictor(const float *y, const int64_t *cls, const float *w, const float *b, int N, float *out, const char *label, hipStream_t s);

}  // namespace fg
}  // namespace pf
