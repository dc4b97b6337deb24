// The weight layouts of the convolution kernels: one writer and one size function per layout (host only; conv_pack.cpp).  Every writer takes
// the conv's folded weights as OIHW fp32 and is called once per conv by build_plan_weights (plan_create.hip); the kernels that read a
// layout say so where they are declared (conv_mfma.h, which includes this file).
#pragma once
#include <cstddef>

namespace pf {

struct ConvTiling;   // conv_mfma.h
struct S4Range;
struct KOrder;       // conv_ranges.h

// ---- host halves of the two-term operand split (conv_mfma.h): fp32 -> fp16 bits, round to nearest even, subnormals kept; and back
unsigned short split_host_f16(float x);
float split_host_f32(unsigned short h);
// 2^k with max|w| * 2^k in [2^14, 2^15) (1 for an all-zero tensor).  Every fp16-pair packer below takes the weights ALREADY multiplied by
// it; the launch's ConvArgs::acc_scale = 1 / that scale
float split_weight_scale(const float *w, size_t n);

// ---- fp32 layouts.  src_ch[n_src]: channels of each input range (sum = cin); K order = the ranges in order, each padded to whole chunks
// of the family's kc channels (zero weights; conv_ranges.h), so a chunk never straddles two source tensors
// generic kernel (conv_mfma.hip): chunks of t.kc channels over the conv's input channels as a whole; floats = t.packed_floats()
void pack_conv_weights(const float *w_oihw, int cin, int cout, const ConvTiling &t, float *out);
// conv_dma.hip: kc = dma_kc(ks, stride)
size_t tiled_packed_floats(const int *src_ch, int n_src, int cout, int ks, int stride);
void pack_conv_weights_tiled(const float *w_oihw, int cin, int cout, int ks, int kc, const int *src_ch, int n_src, float *out);
// ... and its vector-ALU path: the last `rem` (1..16) output channels
size_t rem_packed_floats(const int *src_ch, int n_src, int rem, int ks, int kc);
void pack_conv_weights_rem(const float *w_oihw, int cin, int cout, int rem, int ks, int kc, const int *src_ch, int n_src, float *out);
// conv_wave.hip: kc = wave_kc(ks)
size_t wave_packed_floats(const int *src_ch, int n_src, int cout, int ks);
void pack_conv_weights_wave(const float *w_oihw, int cin, int cout, int ks, const int *src_ch, int n_src, float *out);

// ---- fp16-pair layouts (sizes in floats: the weight arena is a float array)
// conv_split.hip 3x3: chunks of 8 channels; 1x1: chunks of 32
size_t split_packed_floats(const int *src_ch, int n_src, int cout);
void pack_conv_weights_split(const float *w_oihw, int cin, int cout, const int *src_ch, int n_src, float *out);
size_t split1_packed_floats(const int *src_ch, int n_src, int cout);
void pack_conv_weights_split1(const float *w_oihw, int cin, int cout, const int *src_ch, int n_src, float *out);
// conv_s4.hip, conv_front.hip and conv_pair.hip's consumer: K order = the group entries of the ranges of k in order, two entries (8
// channels) per 3x3 round, eight (32 channels) per 1x1 round; weights of channels a range does not own inside its first / last group are
// zero.  pad_sources: every range padded to whole rounds (convs that may be launched one range at a time)
size_t s4_packed_floats(const KOrder &k, int cout, int ks, int pad_sources);
void pack_conv_weights_s4(const float *w_oihw, int cin, int cout, int ks, const KOrder &k, int pad_sources, float *out);
// the fold forms of conv_s4.hip: the 1x1 reader R's weights as [cout tile ntiles][chunk][term][64 lanes][8 fp16] in the folds' K order
// (conv_ranges.h: order_tail, tail_channel); floats = fold_packed_floats(ntiles, chunks) (conv_mfma.h: the kernels size their LDS by it)
void pack_conv_weights_fold(const float *w_oihw, int cin, int cout, const KOrder &k, int ntiles, float *out, int chunks);
// conv_pair.hip: the producer P's weights over its single range r: `two` = [tile][round][2 blocks], `nine` = [tile][round][term][lane][4]
size_t pair_p_two_floats(const S4Range &r, int cout);
size_t pair_p_nine_floats(const S4Range &r, int cout);
void pack_conv_weights_pair_p(const float *w_oihw, int cin, int cout, const S4Range &r, float *two, float *nine);

}  // namespace pf
