// What a caller may ask about a plan or its workspace without running it: workspace size (pf::layout: hardnet_schedule.cpp), the status
// words, taps of intermediate tensors, the flop count; and the packed-pair layout of a single tensor (pf_s4_pack / pf_s4_unpack).
#include <cstring>

#include "hardnet_plan.h"

using namespace pf;

extern "C" int pf_hardnet_workspace(const pf_plan *p, int B, int H, int W, size_t *bytes) {
    if (!p || !bytes || B <= 0 || H <= 0 || W <= 0) return fail(PF_EINVAL, "pf_hardnet_workspace: bad argument");
    std::vector<Dims> d;
    std::vector<size_t> off;
    return layout(p, B, H, W, d, off, *bytes);
}

extern "C" int pf_hardnet_status(const void *ws, unsigned *status, void *stream) {
    if (!ws || !status) return fail(PF_EINVAL, "pf_hardnet_status: null argument");
    PF_HIP_CHECK(hipMemcpyAsync(status, ws, sizeof(unsigned), hipMemcpyDeviceToHost, (hipStream_t)stream));
    PF_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return PF_OK;
}

extern "C" int pf_hardnet_status_sticky(void *ws, unsigned *status, int clear, void *stream) {
    if (!ws || !status) return fail(PF_EINVAL, "pf_hardnet_status_sticky: null argument");
    char *w = (char *)ws + PF_WS_STICKY_OFFSET;
    PF_HIP_CHECK(hipMemcpyAsync(status, w, sizeof(unsigned), hipMemcpyDeviceToHost, (hipStream_t)stream));
    if (clear) {
        int rc = launch_zero_fill(w, sizeof(unsigned), (hipStream_t)stream);
        if (rc) return rc;
    }
    PF_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return PF_OK;
}

extern "C" int pf_hardnet_status_reset(void *ws, void *stream) {
    if (!ws) return fail(PF_EINVAL, "pf_hardnet_status_reset: null argument");
    return launch_zero_fill(ws, PF_WS_STATUS_BYTES, (hipStream_t)stream);
}

extern "C" int pf_hardnet_range_maxima(const pf_plan *p, const void *ws, float *maxima, int cap, int *n_ops, void *stream) {
    if (!p || !ws || !maxima || !n_ops) return fail(PF_EINVAL, "pf_hardnet_range_maxima: null argument");
    *n_ops = (int)p->net.ops.size();
    if (cap < *n_ops) return fail(PF_EINVAL, "pf_hardnet_range_maxima: room for %d values, the plan has %d ops", cap, *n_ops);
    PF_HIP_CHECK(hipMemcpyAsync(maxima, (const char *)ws + (kSlot0 + kMaxSlots) * 4, p->net.ops.size() * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    PF_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return PF_OK;
}

extern "C" int pf_hardnet_tensor_view(const pf_plan *p, const char *name, int B, int H, int W, size_t *ws_offset,
                                      int *channels, int *h, int *w) {
    if (!p || !name || !ws_offset || !channels || !h || !w) return fail(PF_EINVAL, "pf_hardnet_tensor_view: null");
    std::vector<Dims> d;
    std::vector<size_t> off;
    size_t total;
    int rc = layout(p, B, H, W, d, off, total);
    if (rc) return rc;
    for (size_t t = 0; t < p->net.tensors.size(); ++t) {
        if (strncmp(p->net.tensors[t].name, name, sizeof(p->net.tensors[t].name)) == 0) {
            if (off[t] == (size_t)-1) return fail(PF_EINVAL, "tensor '%s' is not materialised", name);
            *ws_offset = off[t];
            *channels = (int)p->net.tensors[t].channels;
            *h = d[t].h;
            *w = d[t].w;
            return PF_OK;
        }
    }
    return fail(PF_EINVAL, "no tensor named '%s'", name);
}

__global__ void unscale_channels_kernel(float *x, const float *inv_scale, int C, size_t hw, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        x[i] *= inv_scale[(i / hw) % C];
}

extern "C" int pf_hardnet_tensor_read(const pf_plan *p, const char *name, int B, int H, int W, const void *ws, float *dst,
                                      void *stream) {
    if (!p || !name || !ws || !dst) return fail(PF_EINVAL, "pf_hardnet_tensor_read: null");
    size_t off;
    int c, h, w;
    int rc = pf_hardnet_tensor_view(p, name, B, H, W, &off, &c, &h, &w);
    if (rc) return rc;
    size_t t = 0;
    while (strncmp(p->net.tensors[t].name, name, sizeof(p->net.tensors[t].name)) != 0) ++t;
    const char *src = (const char *)ws + off;
    if (t < p->last_fmt.size() && p->last_fmt[t] == 0xFF)
        return fail(PF_EUNSUPPORTED, "tensor '%s' was elided by the fused front end (never stored); set plan option fuse_front = 0 to tap it", name);
    if (t < p->last_fmt.size() && p->last_fmt[t] == 0xFE)
        return fail(PF_EUNSUPPORTED, "tensor '%s': its last slice was elided by the tail or lo form of its producer (never stored); set plan options fold_final and fold_lo = 0 to tap it", name);
    if (t < p->last_fmt.size() && p->last_fmt[t]) {
        if ((rc = launch_s4_unpack(src, dst, B, c, h, w, (hipStream_t)stream))) return rc;
    } else {
        int rc = launch_copy(dst, src, (size_t)B * c * h * w * sizeof(float), (hipStream_t)stream);
        if (rc) return rc;
    }
    // tensors are stored multiplied by the plan's per-channel powers of two (normalize_ranges): undo it for the caller
    if (p->inv_scale_off[t]) {
        const size_t n = (size_t)B * c * h * w;
        hipLaunchKernelGGL(unscale_channels_kernel, dim3((unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096)), dim3(256), 0, (hipStream_t)stream,
                           dst, p->dev_weights + p->inv_scale_off[t], c, (size_t)h * w, n);
        PF_LAUNCH_CHECK("unscale_channels_kernel");
    }
    return PF_OK;
}

extern "C" int pf_s4_pack(const float *src, void *dst, int B, int C, int H, int W, unsigned *status, void *stream) {
    if (!src || !dst || B <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(PF_EINVAL, "pf_s4_pack: bad argument");
    return launch_s4_pack(src, dst, B, C, H, W, status, (hipStream_t)stream);
}
extern "C" int pf_s4_unpack(const void *src, float *dst, int B, int C, int H, int W, void *stream) {
    if (!src || !dst || B <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(PF_EINVAL, "pf_s4_unpack: bad argument");
    return launch_s4_unpack(src, dst, B, C, H, W, (hipStream_t)stream);
}

extern "C" int pf_hardnet_flops(const pf_plan *p, int H, int W, double *flops) {
    if (!p || !flops) return fail(PF_EINVAL, "pf_hardnet_flops: null");
    std::vector<Dims> d;
    int rc = propagate_dims(p->net, H, W, d);
    if (rc) return rc;
    double f = 0;
    for (const BlobOp &o : p->net.ops)
        if (o.kind == OP_STEM || o.kind == OP_CONV)
            f += 2.0 * o.cout * d[o.dst].h * d[o.dst].w * o.cin * o.k * o.k;
    *flops = f;
    return PF_OK;
}
