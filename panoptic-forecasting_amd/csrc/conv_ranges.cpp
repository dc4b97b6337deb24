// The K order of a convolution: the order of ranges of each launch form, the chunk / entry counts and the range tables of ConvArgs
// (conv_ranges.h).  Host code only.
#include <cstring>

#include "conv_ranges.h"

namespace pf {

KOrder order_plain(const BlobSrc *src, int n) {
    KOrder k;
    k.n = n;
    int c0 = 0;
    for (int j = 0; j < n; ++j) {
        k.r[j] = KRange{j, src[j].tensor, (int)src[j].choff, (int)src[j].ch, c0};
        c0 += (int)src[j].ch;
    }
    return k;
}

KOrder order_pair(const BlobSrc *src, int n) {
    const KOrder p = order_plain(src, n);
    KOrder k;
    k.n = n;
    for (int j = 0; j < n; ++j) k.r[j] = p.r[(j + 1) % n];
    k.r[n - 1].choff = 0;
    return k;
}

KOrder order_add(const BlobSrc *src, int n) {
    const KOrder p = order_plain(src, n);
    KOrder k;
    k.n = 0;
    for (int j = 0; j < n; ++j)
        if (j != 1) k.r[k.n++] = p.r[j];
    return k;
}

KOrder order_tail(const BlobSrc &src, int slice_choff, int slice_ch) {
    KOrder k;
    k.n = 2;
    const int front = slice_choff - (int)src.choff;
    k.r[0] = KRange{0, src.tensor, (int)src.choff, front, 0};
    k.r[1] = KRange{0, src.tensor, slice_choff, slice_ch, front};
    return k;
}

int tail_channel(const KOrder &k, int chunk, int g, int e) {
    const KRange &r = k.r[chunk == 0 ? 0 : 1];
    // chunk 0: channel (e & 3) of group entry 2g + e / 4 (the range starts on a group); chunk 1: cout 4g + (e & 3) of cout tile e / 4;
    // chunk 2 (three-tile producers): cout 4g + e of cout tile 2 in its low half, nothing above: a lane's D fragments are 4 couts of one
    // pixel per cout tile, so tiles 0 and 1 fill one 8-value K slice and tile 2 half of a second one - no cross-lane traffic
    if (chunk == 2 && e >= 4) return -1;
    const int c = chunk == 0 ? 4 * (2 * g + e / 4) + (e & 3) : chunk == 1 ? 16 * (e / 4) + 4 * g + (e & 3) : 32 + 4 * g + e;
    return c < r.ch ? r.cstart + c : -1;
}

int range_starts(const int *len, int n, int unit, int *out) {
    out[0] = 0;
    for (int j = 0; j < kConvMaxSrc; ++j) out[j + 1] = out[j] + (j < n ? (len[j] + unit - 1) / unit : 0);
    return out[n];
}

int range_chunks(const int *src_ch, int n_src, int kc) {
    int starts[kConvMaxSrc + 1];
    return range_starts(src_ch, n_src, kc, starts);
}

// starts of the ranges' group entries gn[j] (out as range_starts); returns the entries
static int entry_starts(const int *gn, int n, int ks, int pad_sources, int *out) {
    const int per = pad_sources ? s4_per_round(ks) : 1;
    range_starts(gn, n, per, out);
    for (int j = 0; j <= kConvMaxSrc; ++j) out[j] *= per;
    return out[n];
}

int s4_entries(const KOrder &k, int ks, int pad_sources) {
    int gn[kConvMaxSrc], ent0[kConvMaxSrc + 1];
    for (int j = 0; j < k.n; ++j) gn[j] = s4_range_groups(k.r[j].choff, k.r[j].ch);
    return entry_starts(gn, k.n, ks, pad_sources, ent0);
}

int s4_rounds(const KOrder &k, int ks, int pad_sources) {
    const int per = s4_per_round(ks);
    return (s4_entries(k, ks, pad_sources) + per - 1) / per;
}

int set_chunks(ConvArgs &a, int kc) {
    int ch[kConvMaxSrc];
    for (int j = 0; j < a.n_src; ++j) ch[j] = a.src_cstart[j + 1] - a.src_cstart[j];
    const int chunks = range_starts(ch, a.n_src, kc, a.src_chunk0);
    a.chunk_begin = a.src_chunk0[a.src_begin];
    a.chunk_end = a.src_chunk0[a.src_end];
    return chunks;
}

int set_s4_entries(ConvArgs &a, int ks, int pad_sources) {
    const int per = s4_per_round(ks);
    for (int j = 0; j < a.n_src; ++j) {
        a.src_c4[j] = (a.src_ctotal[j] + 3) / 4;
        a.src_g0[j] = a.src_choff[j] / 4;
        a.src_gn[j] = s4_range_groups(a.src_choff[j], a.src_cstart[j + 1] - a.src_cstart[j]);
    }
    const int entries = entry_starts(a.src_gn, a.n_src, ks, pad_sources, a.src_ent0);
    a.chunk_begin = a.src_ent0[a.src_begin] / per;
    a.chunk_end = (a.src_ent0[a.src_end] + per - 1) / per;
    return (entries + per - 1) / per;
}

}  // namespace pf

// one case of pf_debug_conv_ranges
static int debug_conv_ranges(int form, int ks, int kc, int pad, int n_src, const int *choff, const int *ch, const int *ctotal, int src_begin, int src_end,
                             int *out) {
    using namespace pf;
    BlobSrc src[kConvMaxSrc];
    for (int j = 0; j < n_src; ++j) src[j] = BlobSrc{(uint32_t)j, (uint32_t)choff[j], (uint32_t)ch[j]};
    const KOrder k = form == 0 ? order_plain(src, n_src) : (form == 1 ? order_pair(src, n_src) : order_add(src, n_src));
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    set_sources(a, k, [&](uint32_t t) { return TensorRef{nullptr, ctotal[t]}; });
    if (src_begin >= 0 && src_end > src_begin && src_end <= a.n_src) { a.src_begin = src_begin; a.src_end = src_end; }
    const int count = kc > 0 ? set_chunks(a, kc) : set_s4_entries(a, ks, pad);
    if (kc == 0 && count != s4_rounds(k, ks, pad)) return fail(PF_EINVAL, "pf_debug_conv_ranges: the filler and s4_rounds disagree");
    memset(out, 0, 39 * sizeof(int));
    out[0] = k.n; out[1] = count;
    for (int j = 0; j < k.n; ++j) { out[2 + j] = k.r[j].src; out[11 + j] = k.r[j].cstart; }
    memcpy(out + 6, a.src_cstart, sizeof(a.src_cstart));
    memcpy(out + 15, a.src_chunk0, sizeof(a.src_chunk0));
    memcpy(out + 20, a.src_c4, sizeof(a.src_c4));
    memcpy(out + 24, a.src_g0, sizeof(a.src_g0));
    memcpy(out + 28, a.src_gn, sizeof(a.src_gn));
    memcpy(out + 32, a.src_ent0, sizeof(a.src_ent0));
    out[37] = a.chunk_begin; out[38] = a.chunk_end;
    return PF_OK;
}

extern "C" int pf_debug_conv_ranges(int form, int ks, int kc, int pad, int n_src, int n_cases, const int *choff, const int *ch, const int *ctotal,
                                    int src_begin, int src_end, int *out, size_t cap) {
    if (!choff || !ch || !ctotal || !out || n_cases < 0 || cap < (size_t)n_cases * 39)
        return pf::fail(PF_EINVAL, "pf_debug_conv_ranges: null argument or fewer than 39 ints of output per case");
    if (form < 0 || form > 2 || n_src < (form ? 2 : 1) || n_src > pf::kConvMaxSrc || (ks != 1 && ks != 3) || kc < 0)
        return pf::fail(PF_EINVAL, "pf_debug_conv_ranges: form %d, %d ranges, ks %d, kc %d", form, n_src, ks, kc);
    for (int i = 0; i < n_cases; ++i) {
        const size_t r = (size_t)i * pf::kConvMaxSrc;
        const int rc = debug_conv_ranges(form, ks, kc, pad, n_src, choff + r, ch + r, ctotal + r, src_begin, src_end, out + (size_t)i * 39);
        if (rc) return rc;
    }
    return PF_OK;
}
