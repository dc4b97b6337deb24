// fg forecaster: pf_fg_pack - the raw state_dict copy, the [tile][K][64] GEMM weights behind it and, under PF_FG_PAIR, the fp16-pair
// section (fg_net.h: Layout, PairLayout).
#include "fg_net.h"

namespace pf {
namespace fg {

// packed[tile][k][q] = W[row(tile, q)][k]  (MAP_LSTM: row = gate*256 + tile*16 + q%16, gate = q/16; MAP_PLAIN: row = tile*64+q);
// MAP_KMAJOR (ConvTranspose2d [cin][cout*4]): packed[tile][k][q] = W[k][tile*64 + q]
__global__ __launch_bounds__(256) void pack_kernel(const float *__restrict__ w, float *__restrict__ out, int K, int tiles, int map) {
    const long long total = (long long)tiles * K * 64;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int q = (int)(i & 63);
        const long long tk = i >> 6;
        const int k = (int)(tk % K), tile = (int)(tk / K);
        float v;
        if (map == MAP_KMAJOR) {
            v = w[(long long)k * tiles * 64 + tile * 64 + q];
        } else {
            const int row = map == MAP_LSTM ? (q >> 4) * C + tile * 16 + (q & 15) : tile * 64 + q;
            v = w[(long long)row * K + k];
        }
        out[i] = v;
    }
}

// The pair section's scale: k = the rule of split_weight_scale (conv_mfma.h): max |w * 2^k| in [2^14, 2^15), k = 0 for an all-zero (or
// non-finite) tensor; the weights live on the device, so the maximum is a reduction kernel and k is derived from it by every packing
// thread.  |k| <= 120 keeps 2^k and 2^-k normal numbers (a tensor whose maximum is below 2^-106 is then scaled less than the rule says;
// both scalings stay exact)
__global__ __launch_bounds__(256) void absmax_kernel(const float *__restrict__ w, long long n, unsigned *__restrict__ out) {
    __shared__ unsigned m;
    if (threadIdx.x == 0) m = 0u;
    __syncthreads();
    float v = 0.f;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) v = fmaxf(v, fabsf(w[i]));
    atomicMax(&m, __builtin_bit_cast(unsigned, v));
    __syncthreads();
    if (threadIdx.x == 0 && m != 0u) atomicMax(out, m);
}

__device__ __forceinline__ int pair_exponent(unsigned maxbits) {
    const float m = __builtin_bit_cast(float, maxbits);
    if (!(m > 0.f) || !(m <= 3.4028234e38f)) return 0;
    const int k = 14 - ilogbf(m);
    return k < -120 ? -120 : (k > 120 ? 120 : k);
}

__global__ __launch_bounds__(256) void pack_pair_kernel(const float *__restrict__ w, _Float16 *__restrict__ out, int ctot, int tiles, int map,
                                                        const unsigned *__restrict__ maxbits, float *__restrict__ scale) {
    const int k = pair_exponent(*maxbits);
    if (blockIdx.x == 0 && threadIdx.x == 0) *scale = ldexpf(1.f, -k);
    const int rounds = (ctot + PKC - 1) / PKC, K = ctot * 9;
    const long long total = (long long)tiles * rounds * PTERM_W;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % PKC), q = (int)(i / PKC % 64);
        const long long t = i / (64 * PKC);
        const int tap = (int)(t % 9);
        const long long tr = t / 9;
        const int round = (int)(tr % rounds), tile = (int)(tr / rounds);
        const int c = round * PKC + ch;
        float v = 0.f;
        if (c < ctot) {
            const int row = map == MAP_LSTM ? (q >> 4) * C + tile * 16 + (q & 15) : tile * 64 + q;
            v = ldexpf(w[(long long)row * K + c * 9 + tap], k);
        }
        const _Float16 hi = (_Float16)v;
        const _Float16 mid = (_Float16)(v - (float)hi);
        const long long at = tr * PROUND + (tap * 64 + q) * PKC + ch;
        out[at] = hi;
        out[at + PTERM_W] = mid;
    }
}

}  // namespace fg
}  // namespace pf

using namespace pf;
using namespace pf::fg;

extern "C" int pf_fg_pack(const float *raw, float *packed, int flags, void *stream) {
    if (int rc = check_dims(0, 1, 1, flags)) return rc;
    if (!raw || !packed) return fail(PF_EINVAL, "pf_fg_pack: null buffer");
    hipStream_t s = (hipStream_t)stream;
    const Layout L = layout();
    if (int rc = launch_copy(packed, raw, L.raw_total * sizeof(float), s)) return rc;
    for (int g = 0; g < NGEMM; ++g) {
        const GemmDesc &d = kGemm[g];
        hipLaunchKernelGGL(pack_kernel, dim3(1024), dim3(256), 0, s, raw + L.raw[d.src], packed + L.gemm[g], d.ctot * d.taps,
                           d.tiles, d.map);
        PF_LAUNCH_CHECK("pf_fg_pack");
    }
    if (flags & PF_FG_PAIR) {
        const PairLayout P = pair_layout(L);
        unsigned *head = reinterpret_cast<unsigned *>(packed + P.head);
        if (int rc = launch_zero_fill(head, 64 * sizeof(float), s)) return rc;
        for (int i = 0; i < NPAIR; ++i) {
            const GemmDesc &d = kGemm[kPairGemm[i]];
            const long long n = (long long)d.tiles * 64 * d.ctot * d.taps;
            hipLaunchKernelGGL(absmax_kernel, dim3(256), dim3(256), 0, s, raw + L.raw[d.src], n, head + i);
            PF_LAUNCH_CHECK("pf_fg_pack");
            hipLaunchKernelGGL(pack_pair_kernel, dim3(1024), dim3(256), 0, s, raw + L.raw[d.src], reinterpret_cast<_Float16 *>(packed + P.gemm[i]),
                               d.ctot, d.tiles, d.map, head + i, packed + P.head + 8 + i);
            PF_LAUNCH_CHECK("pf_fg_pack");
        }
    }
    return 0;
}
