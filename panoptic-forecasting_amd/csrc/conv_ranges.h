// The K order of a convolution (host only; conv_ranges.cpp).  A conv reads its input as up to kConvMaxSrc channel ranges of earlier
// tensors and every kernel family walks them the same way: the ranges of the launch in order, each padded to whole chunks of the
// family's kc channels - for the packed-pair kernels to whole group entries, and to whole rounds where the conv was packed with
// pad_sources.  The packers and the schedules take the order of a launch form and every table derived from it from here.
#pragma once
#include "conv_mfma.h"

namespace pf {

// One range of a launch
struct KRange {
    int src;           // which range of the op it is
    uint32_t tensor;   // the tensor it lives in
    int choff, ch;     // its first channel inside that tensor as the launch addresses it, and its channels
    int cstart;        // its first input channel in the op's weight numbering
};
// The ranges of one launch in K order
struct KOrder {
    int n;
    KRange r[kConvMaxSrc];
};
// the op's ranges as they are
KOrder order_plain(const BlobSrc *src, int n);
// conv_pair.hip: the consumer C = conv(P ++ S ++ others) as [S, others.., P], P's output declared at channel 0 of its own planes
KOrder order_pair(const BlobSrc *src, int n);
// the add launch of conv_s4.hip: the same consumer without S, its range 1
KOrder order_add(const BlobSrc *src, int n);
// the fold forms of conv_s4.hip (tail, down): the single range of a 1x1 reader R, cut at the slice [slice_choff, slice_choff + slice_ch) that ends it:
// [R's other channels (in front of the slice; may be empty), the slice]
KOrder order_tail(const BlobSrc &src, int slice_choff, int slice_ch);
// ... and its K order: R's input channel at K position e (0..7) of lane group g in chunk 0 (the other channels: group entries 2g and
// 2g + 1 of range 0, four channels each) or chunk 1 (the slice as the producing launch holds it: couts 4g .. 4g + 3 of its first cout
// tile, then of its second) or, for a producer of three cout tiles, chunk 2 (couts 4g .. 4g + 3 of its third cout tile at e = 0..3,
// nothing at e = 4..7); -1 = no channel (the weight is zero)
int tail_channel(const KOrder &k, int chunk, int g, int e);

// starts of n ranges of len[j] elements, each padded to whole units of `unit`, counted in units: out[j] for j <= kConvMaxSrc (out[n]
// and the tail = the total, which is returned)
int range_starts(const int *len, int n, int unit, int *out);
// chunks of kc channels of a conv over ranges of src_ch[j] channels (kc per family: dma_kc, wave_kc, 8 / 32 for conv_split)
int range_chunks(const int *src_ch, int n_src, int kc);
// group entries of a packed-pair launch (one 4-channel group of one range; two per 3x3 round, eight per 1x1 round); pad_sources: every
// range padded to whole rounds (convs that may run one range at a time: the halves of a commuted upsample + 1x1, and conv_pair)
inline int s4_per_round(int ks) { return ks == 3 ? 2 : 8; }
inline int s4_range_groups(int choff, int ch) { return (choff + ch + 3) / 4 - choff / 4; }
int s4_entries(const KOrder &k, int ks, int pad_sources);
int s4_rounds(const KOrder &k, int ks, int pad_sources);

// ---- a launch's ConvArgs.  What only a schedule knows of a tensor comes from it: tensor_ref(tensor) -> TensorRef
struct TensorRef {
    const float *base;
    int channels;
};
// src, src_ctotal, src_choff, src_cstart (prefix sums in the launch's own order; the tail = their total), n_src, src_begin = 0, src_end = n_src
template <typename F>
void set_sources(ConvArgs &a, const KOrder &k, F tensor_ref) {
    int ch[kConvMaxSrc];
    for (int j = 0; j < k.n; ++j) {
        const TensorRef t = tensor_ref(k.r[j].tensor);
        a.src[j] = t.base;
        a.src_ctotal[j] = t.channels;
        a.src_choff[j] = k.r[j].choff;
        ch[j] = k.r[j].ch;
    }
    range_starts(ch, k.n, 1, a.src_cstart);
    a.n_src = k.n;
    a.src_begin = 0;
    a.src_end = k.n;
}
// src_chunk0 for chunks of kc channels, chunk_begin / chunk_end of the ranges [src_begin, src_end); returns the conv's chunks
int set_chunks(ConvArgs &a, int kc);
// src_c4, src_g0, src_gn, src_ent0 of packed-pair sources, chunk_begin / chunk_end in rounds; returns the conv's rounds
int set_s4_entries(ConvArgs &a, int ks, int pad_sources);

}  // namespace pf
