// fg forecaster: pf_fg_forward - checks the arguments, takes the schedule (fg_schedule.cpp: every launch and its buffers), resolves its
// regions to pointers and enqueues the steps in order - and the two status calls of a PF_FG_PAIR workspace.
#include "fg_net.h"

using namespace pf;
using namespace pf::fg;

extern "C" int pf_fg_forward(const float *packed, int flags, int N, int T_in, int T_out, int odom_T, const float *trajs,
                             const float *traj_mask, const float *vel_mask, const float *feats, const int64_t *output_inds,
                             const float *odom, const float *depths, const float *depth_mask, const int64_t *classes,
                             float *traj_norm, float *traj_unnorm, float *mask_feats, float *output_feats, float *masks,
                             void *ws, size_t ws_bytes, void *stream) {
    if (int rc = check_dims(N, T_in, T_out, flags)) return rc;
    if (odom_T < T_in + T_out) return fail(PF_EINVAL, "pf_fg_forward: odometry has %d steps, needs T_in + T_out = %d", odom_T, T_in + T_out);
    const Ws W = ws_layout(N, T_in, flags);
    if (N == 0) return 0;      // nothing to forecast: no launch
    if (!packed || !trajs || !traj_mask || !vel_mask || !feats || !output_inds || !odom || !depths || !depth_mask || !classes ||
        !traj_norm || !traj_unnorm || !mask_feats || !output_feats || !masks || !ws)
        return fail(PF_EINVAL, "pf_fg_forward: null buffer");
    if (ws_bytes < W.total) return fail(PF_EWORKSPACE, "pf_fg_forward: workspace %zu < %zu bytes", ws_bytes, W.total);
    std::vector<Step> steps;
    if (int rc = build_fg_schedule(N, T_in, T_out, flags, steps)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Layout L = layout();
    const PairLayout PL = pair_layout(L);
    const float *R = packed;
    unsigned *status = (unsigned *)ws;

    float *base[NREGION] = {};      // feats is only ever an x operand: read
    for (int r = R_STATUS; r < R_FEATS; ++r) base[r] = (float *)ws + W.off[r];
    base[R_FEATS] = const_cast<float *>(feats), base[R_MASK_FEATS] = mask_feats, base[R_OUTPUT_FEATS] = output_feats, base[R_MASKS] = masks;
    auto at = [&](const Operand &o) { return o.region ? base[o.region] + o.off : nullptr; };

    TrajArgs ta = {};
    ta.trajs = trajs, ta.traj_mask = traj_mask, ta.vel_mask = vel_mask, ta.depths = depths, ta.depth_mask = depth_mask;
    ta.odom = odom, ta.T_in = T_in, ta.T_out = T_out, ta.odom_T = odom_T;
    ta.traj_norm = traj_norm, ta.traj_unnorm = traj_unnorm;
    ta.odom_mean = R + L.raw[ODOM_MEAN], ta.odom_std = R + L.raw[ODOM_STD];
    ta.depth_mean = R + L.raw[DEPTH_MEAN], ta.depth_std = R + L.raw[DEPTH_STD];
    ta.traj_mean = R + L.raw[TRAJ_MEAN], ta.traj_std = R + L.raw[TRAJ_STD];
    ta.wtf = R + L.raw[TFO_W], ta.btf = R + L.raw[TFO_B];

    for (const Step &st : steps) {
        int rc = 0;
        switch (st.kind) {
            case K_STATUS: rc = launch_status(status, 1, s); break;
            case K_INST_FEAT:       // the encoder's launch covers the T_in planes of an instance, each times its step mask
                rc = st.t < 0 ? launch_inst_feat(at(st.x), st.x.stride, (long long)C * HW, traj_mask, N, T_in, R, L, at(st.out), st.label, s)
                              : launch_inst_feat(at(st.x), st.x.stride, 0LL, nullptr, N, 1, R, L, at(st.out), st.label, s);
                break;
            case K_TRAJ_ENC: case K_TRAJ_DEC: {
                const bool dec = st.kind == K_TRAJ_DEC;
                const int w = dec ? TD_WIH : TE_WIH, o = dec ? TDO_W0 : TEO_W0;      // W_ih, W_hh, b_ih, b_hh / W0, b0, W2, b2 follow each other
                TrajArgs a = ta;
                a.instf = at(st.x), a.tfeat = at(st.out), a.gru_h = at(st.c), a.step = dec ? st.t : 0;
                a.wih = R + L.raw[w], a.whh = R + L.raw[w + 1], a.bih = R + L.raw[w + 2], a.bhh = R + L.raw[w + 3];
                a.w0 = R + L.raw[o], a.b0 = R + L.raw[o + 1], a.w2 = R + L.raw[o + 2], a.b2 = R + L.raw[o + 3];
                rc = launch_traj(a, dec, N, st.label, s);
                break;
            }
            case K_GEMM: case K_PAIR: {
                const GemmDesc &d = kGemm[st.gemm];
                fg::PairArgs pa = {};
                GemmArgs &g = pa.g;
                g.vec = at(st.vec), g.vec_stride = st.vec.stride, g.nvec = st.nvec;
                g.x = at(st.x), g.x_stride = st.x.stride, g.nx = st.nx;
                g.h = at(st.h), g.h_stride = st.h.stride, g.nh = st.nh;
                g.ctot = d.ctot, g.w = R + L.gemm[st.gemm], g.bias = R + L.raw[d.src + 1];
                g.out = at(st.out), g.out_stride = st.out.stride, g.c = at(st.c);
                if (st.kind == K_GEMM) {
                    rc = launch_gemm(g, d.taps, st.epi, N, d.tiles, st.label, s);
                    break;
                }
                pa.wp = reinterpret_cast<const split_t *>(R + PL.gemm[st.pair]), pa.scale = R + PL.head + 8 + st.pair;
                pa.status = status, pa.slots = status + FG_SLOT0 + 3 * st.slot;
                rc = launch_pair(pa, st.epi, N, d.tiles, st.label, s);
                break;
            }
            case K_GATHER: rc = launch_gather(at(st.x), output_inds, N, T_out, at(st.out), s); break;
            case K_PREDICT: rc = launch_predictor(at(st.x), classes, R + L.raw[PR_W], R + L.raw[PR_B], N, at(st.out), st.label, s); break;
        }
        if (rc) return rc;
    }
    return 0;
}

extern "C" int pf_fg_status(void *ws, unsigned *out2, void *stream) {
    if (!ws || !out2) return fail(PF_EINVAL, "pf_fg_status: null argument");
    hipStream_t s = (hipStream_t)stream;
    unsigned *st = (unsigned *)ws;
    if (int rc = launch_status(st, 0, s)) return rc;
    if (hipMemcpyAsync(out2, st + 2, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(PF_EHIP, "pf_fg_status: reading the status words failed");
    return 0;
}

extern "C" int pf_fg_status_reset(void *ws, void *stream) {
    if (!ws) return fail(PF_EINVAL, "pf_fg_status_reset: null workspace");
    return launch_zero_fill(ws, FG_STATUS_WORDS * sizeof(unsigned), (hipStream_t)stream);
}
