// What a training step prepares before its first convolution: the dense one-hot + depth input tensor and the tiled weight
// packings of all its forward and backward-data convolutions.
#include "train_kernels.h"

namespace pf {

// ------------------------------------------------------------------------------------------------ input: one-hot + depth
// bg_model.py:53-69: labels >= n_cls -> zero vector; depth channels = (d - mean) / std * mask, after the T one-hot groups
__global__ __launch_bounds__(256) void onehot_dense_kernel(const void *seg, int seg_i64, const float *depth, const uint8_t *mask,
                                                           float mean, float stdv, int B, int T, int n_cls, long long HW, float *x) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int bt = blockIdx.y, b = bt / T, t = bt - b * T;
    if (i >= HW) return;
    const long long in = (long long)bt * HW + i;
    const long long lab = seg_i64 ? reinterpret_cast<const long long *>(seg)[in] : (long long)reinterpret_cast<const uint8_t *>(seg)[in];
    const int C = T * (n_cls + 1);
    float *xb = x + (long long)b * C * HW + i;
    for (int c = 0; c < n_cls; ++c) xb[(long long)(t * n_cls + c) * HW] = (lab == c) ? 1.f : 0.f;
    const float dn = (depth[in] - mean) / stdv;
    xb[(long long)(T * n_cls + t) * HW] = dn * (mask[in] ? 1.f : 0.f);
}

int launch_onehot_dense(const void *seg, int seg_i64, const float *depth, const uint8_t *mask, float mean, float stdv, int B, int T,
                        int n_cls, int H, int W, float *x, hipStream_t s) {
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(onehot_dense_kernel, dim3((unsigned)((HW + 255) / 256), B * T), dim3(256), 0, s, seg, seg_i64, depth, mask, mean,
                       stdv, B, T, n_cls, HW, x);
    PF_LAUNCH_CHECK("onehot_dense_kernel");
    return PF_OK;
}

// ------------------------------------------------------------------------------------------------ weight packing on the device
// OIHW -> the per-tile order of the LDS-DMA kernels (conv_pack.cpp: pack_conv_weights_tiled, [cout tile][chunk][kgroup][tap][64 lanes],
// K order = the input ranges in order, each padded to whole chunks of kc channels).
// transpose_flip = 0: forward weights.  transpose_flip = 1: the backward-data convolution of input range [c0, c0+ch):
//   Wd[co_d][ci_d][tap] = W[ci_d][c0 + co_d][ks2-1-tap]   (ci_d runs over the forward cout)
// which has ONE input range (the forward cout channels of dy).
// All tiled packings of a training step in a handful of launches (train_plan.hip collects the jobs: one per forward conv, one per
// backward-data conv): a step used to spend 190 launches of ~4.6 us on them (0.87 ms of a 20.7 ms step).  The jobs travel as kernel
// arguments, kPackBatch per launch; a workgroup finds its job by a scalar walk over the block prefix
__global__ __launch_bounds__(256) void pack_weights_batch_kernel(const float *theta, float *arena, PackBatch pb) {
    int j = 0;
    while (j + 1 < pb.n && (int)blockIdx.x >= pb.job[j + 1].block0) ++j;
    const PackJob &q = pb.job[j];
    const long long o = (long long)((int)blockIdx.x - q.block0) * 256 + threadIdx.x;
    if (o >= q.total) return;
    const float *w = theta + q.w_off;
    const int nchunks = q.chunk0[q.n_src];
    long long r = o;
    const int lane = (int)(r % 64); r /= 64;
    const int tap = (int)(r % q.ks2); r /= q.ks2;
    const int kg = (int)(r % (q.kc / 4)); r /= (q.kc / 4);
    const int chunk = (int)(r % nchunks); r /= nchunks;
    const int t = (int)r;
    int jj = 0;
    while (jj + 1 < q.n_src && chunk >= q.chunk0[jj + 1]) ++jj;
    const int cl = (chunk - q.chunk0[jj]) * q.kc + kg * 4 + (lane >> 4), nch = q.cstart[jj + 1] - q.cstart[jj];
    const int co = t * 16 + (lane & 15), ci = q.cstart[jj] + cl;
    float v = 0.f;
    if (cl < nch) {
        if (!q.tflip) {
            if (co < q.cout_f) v = w[((long long)co * q.cin_f + ci) * q.ks2 + tap];
        } else {
            if (co < q.ch) v = w[((long long)ci * q.cin_f + q.c0 + co) * q.ks2 + (q.ks2 - 1 - tap)];   // ci runs over the forward cout
        }
    }
    arena[q.out_off + o] = v;
}
void pack_job_fill(PackJob &q, size_t w_off, int cin_f, int cout_f, int ks, int stride, const int *src_ch, int n_src, int transpose_flip, int c0,
                   int ch, size_t out_off) {
    const int kc = dma_kc(ks, stride);
    q.w_off = (long long)w_off; q.out_off = (long long)out_off;
    q.cin_f = cin_f; q.cout_f = cout_f; q.ks2 = ks * ks; q.kc = kc; q.tflip = transpose_flip; q.c0 = c0; q.ch = ch; q.n_src = n_src;
    range_starts(src_ch, n_src, 1, q.cstart);
    range_starts(src_ch, n_src, kc, q.chunk0);
    q.total = (long long)tiled_packed_floats(src_ch, n_src, transpose_flip ? ch : cout_f, ks, stride);
    q.block0 = 0;
}
int launch_pack_weights_batch(const float *theta, float *arena, const PackJob *jobs, int n, hipStream_t s) {
    for (int i0 = 0; i0 < n; i0 += kPackBatch) {
        PackBatch pb;
        pb.n = n - i0 < kPackBatch ? n - i0 : kPackBatch;
        int blocks = 0;
        for (int k = 0; k < pb.n; ++k) {
            pb.job[k] = jobs[i0 + k];
            pb.job[k].block0 = blocks;
            blocks += (int)((jobs[i0 + k].total + 255) / 256);
        }
        if (blocks == 0) continue;
        hipLaunchKernelGGL(pack_weights_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, s, theta, arena, pb);
        PF_LAUNCH_CHECK("pack_weights_batch_kernel");
    }
    return PF_OK;
}

}  // namespace pf
