// Per-layer choice between the two fp32 MFMA convolution kernels and their tile shapes.
#include "conv_mfma.h"

namespace pf {

namespace {
ConvChoice g_conv_force = {CONV_AUTO, 0, 0, 0};   // pf_debug_force_conv
struct Tuned {
    int ks, cin, cout, hout, wout, B;
    ConvChoice c;
};
// Measured winners for the shapes of the 1024x2048 bg network (tools/tune_convs.py --emit on an MI355X); rows are
// only kept where they beat the cost model by > 3 %.
const Tuned kTuned[] = {
#include "conv_tuned.inc"
};

// conv_s4 (packed-pair sources): measured per-layer shapes with every eligible layer on conv_s4 (tools/tune_s4.py --emit).
// kind 5 (CONV_S4) = run it on conv_s4 with (p0 = cout tiles per workgroup, p1 = S4Tile) if the plan can give it S4 sources,
// kind 0 (CONV_AUTO) = the table's fp32-source kernel measured faster in situ: do not ask for S4 sources.
const Tuned kTunedS4[] = {
    {0, 0, 0, 0, 0, 0, {0, 0, 0, 0}},
#include "conv_s4_tuned.inc"
};

}  // namespace

// A layer of the architecture at an image size the tables were not measured at.  Both tables are keyed on the exact shapes of the
// 1024x2048 network; what a row's choice depends on is how many tiles its launch has, i.e. its pixel count B * hout * wout, not
// the image size as such (every kernel clips its tiles at the image edge).  So the layer (ks, cin, cout) - each occurs at ONE
// resolution of the measured network, and the conv_s4 table has a row for every layer at every measured batch - is looked up
// with the batch size at which the measured launch had the same number of pixels: 512x1024 at B = 16 takes the B = 4 rows.
// Launches with less than half the pixels of the smallest measured one (B = 1) are outside what the rows know: heuristics.
// Returns false when the layer is not in the table at all (another architecture) or that small; *exact = its measured size is this one.
namespace {
bool measured_geometry(int ks, int cin, int cout, int hout, int wout, int B, int *ht, int *wt, double *b_eq, bool *exact) {
    // a row measured at exactly this size wins over any other resolution of the same (ks, cin, cout) (today every layer occurs at one
    // resolution - tests/test_host_logic.py asserts it on both tables - but a table that gains a second size must not remap the first)
    const Tuned *first = nullptr;
    for (const Tuned &t : kTunedS4) {
        if (t.B <= 0 || t.ks != ks || t.cin != cin || t.cout != cout) continue;
        if (t.hout == hout && t.wout == wout) {
            *ht = hout;
            *wt = wout;
            *exact = true;
            *b_eq = (double)B;
            return true;
        }
        if (!first) first = &t;
    }
    if (!first) return false;
    *ht = first->hout;
    *wt = first->wout;
    *exact = false;
    *b_eq = (double)B * hout * wout / ((double)first->hout * first->wout);
    return *b_eq >= 0.5;
}
}  // namespace

// Row of the conv_s4 table for this layer at the measured batch size nearest to B (in ratio); false: no row at all.
bool choose_s4(int ks, int cin, int cout, int hout, int wout, int B, ConvChoice *out) {
    int ht, wt;
    double b_eq;
    bool exact;
    if (!measured_geometry(ks, cin, cout, hout, wout, B, &ht, &wt, &b_eq, &exact)) return false;
    const Tuned *best = nullptr;
    double best_d = 0.0;
    for (const Tuned &t : kTunedS4) {
        if (t.ks != ks || t.cin != cin || t.cout != cout || t.hout != ht || t.wout != wt || t.B <= 0) continue;
        const double d = t.B > b_eq ? (double)t.B / b_eq : b_eq / (double)t.B;
        if (!best || d < best_d || (d == best_d && t.B > best->B)) { best = &t; best_d = d; }
    }
    if (!best) return false;
    *out = best->c;
    return true;
}

// conv_pair.hip (an odd HarDBlock layer inside its consumer) instead of two conv_s4 launches?  mode = plan option fuse_pairs: 0 never,
// 2 wherever the kernel exists (tests, A/B runs), 1 (default) where it MEASURED faster (MI355X, 1024x2048 network, per pair, same box:
// profiles/r06_experiments.md).  The fused form does 1.17-1.21x the matrix work of the two launches (the odd layer on 360 + 24 positions
// per 256 pixels) for 0.68x their bytes, and both forms run at the same ~60 % of the matrix pipe's sustained rate - the pipe and the
// LDS fragment reads bound them, not the DMA the fusion saves - so a full chip loses exactly the extra matrix work:
//      pixels of the launch (B * H * W)   524 288+ (B >= 4 at 256x512)    131 072 (B = 1 at 256x512, B = 4 at 128x256)     32 768
//      <2, 1> pairs (C <= 32, P <= 16)    1.06 - 1.31 x the two launches   0.84 - 0.96 x                                    0.97 - 1.15
//      <3, 1> / <*, 2> pairs              1.3 - 2.8 x (register spills at 128 registers per lane)
// It wins where the chip is NOT full: one launch of 512 eight-wave workgroups instead of two launches of 512 four-wave ones.
bool pair_wanted(int p_cin, int p_cout, int c_cin, int c_cout, int h, int w, int B, int mode) {
    if (mode == 4) return conv_pair_merged_supports(c_cout, p_cout);
    if (mode >= 2) return true;
    if (mode <= 0) return false;
    const long px = (long)B * h * w;
    return c_cout <= 32 && p_cout <= 16 && px >= 65536 && px <= 196608;
}

// conv_s4.hip share / add instead of the two plain launches of a pair?  mode = plan option share_s: 0 never, 2 wherever the forms exist
// (tests, A/B runs), 1 (default): where the packed rows (P's couts rounded up to 4, then C's) need fewer cout tiles than the two launches
// together, outside the window in which pair_wanted selects conv_pair, and only for the pairs whose share + add launches MEASURED faster
// than the two plain ones in every run (MI355X, 1024x2048 network, B = 32 per launch, same box: profiles/r07_experiments.md)
bool share_wanted(int p_cin, int p_cout, int c_cin, int c_cout, int h, int w, int B, int mode) {
    if (mode >= 2) return true;
    if (mode <= 0) return false;
    const int packed = (share_row0(p_cout) + c_cout + 15) / 16, apart = (p_cout + 15) / 16 + (c_cout + 15) / 16;
    if (packed >= apart || pair_wanted(p_cin, p_cout, c_cin, c_cout, h, w, B, 1)) return false;
    // the measured winners: 48 -> 10 -> 18 (635-637 -> 534-547 us) and 63 -> 10 -> 18 (772-775 -> 605-623 us) at 256x512, B = 32: launches
    // of 4 M pixels, S of 48 channels or more.  The two (24, 40) pairs of the 32x64 level (four tiles instead of five) gained 3-5 us of 45
    // each in every run, 0.06 % of a step and a fifth of the headline's own spread: they stay as they are; every other pair of the
    // network packs no tile away or measured slower
    return p_cout == 10 && c_cout == 18 && p_cin >= 48 && (long)B * h * w >= 4194304;
}

// conv_s4.hip tail (a 3x3 conv's launch also computes the 1x1 conv that alone reads its slice) instead of the two plain launches?  mode =
// plan option fold_final: 0 never, 2 wherever the form exists (tests, A/B runs), 1 (default): only the class of launches whose folded
// runs MEASURED faster than the two plain launches in every run (MI355X, 1024x2048 network, same box, fold_final 0 / 2 alternated:
// profiles/r08_experiments.md): 91 -> 28 -> 11 at 256x512, B = 4 .. 32 - 99 -> 75 us, 200 -> 150 us, .., 745-755 -> 576-579 us: the 1x1
// launch's time less 2-3 % of the 3x3 launch's.  Launches of more than 4 194 304 pixels and other channel counts were not measured and
// keep their two launches; B = 2 (262 144 pixels) won too, 57 -> 42 us in both of its runs, and is left out: the parity and suite runs
// of the change were made with the rule as it stands (B = 1 lies in pair_wanted's window: that layer runs inside conv_pair)
bool tail_wanted(int cin, int cout, int r_cout, int h, int w, int B, int mode) {
    if (mode >= 2) return true;
    if (mode <= 0) return false;
    const long px = (long)B * h * w;
    return cin == 91 && cout == 28 && r_cout == 11 && px >= 524288 && px <= 4194304;
}

// conv_s4.hip down (a 3x3 conv's launch also computes the 1x1 conv + 2x2 average pool behind it) instead of the two launches?  mode = plan
// option fold_down: 0 never, 2 wherever the form exists (tests, A/B runs), 1 (default): only the class of launches whose folded runs
// MEASURED faster than the two launches in every run (MI355X, 1024x2048 network, same box, fold_down 0 / 2 alternated three times:
// profiles/r09_experiments.md): 76 -> 28 -> 64 at 256x512, B = 4 .. 32 - 103 -> 79 us, 205-207 -> 164-165 us, 393-401 -> 317-324 us,
// 781-790 -> 640-642 us: the folded launch takes the 3x3 launch's time and about half of the 1x1 launch's.  And the three-tile form
// (profiles/r10_experiments.md, the same protocol): 108 -> 46 -> 96 at 128x256, B = 4 .. 32 - 67-69 -> 52-54 us, 108-109 -> 89-91 us,
// 201-202 -> 164-166 us, 393-397 -> 315-322 us.  Other channel counts, smaller launches (B = 1, 2) and larger ones than the measured
// were not measured and keep their two launches
bool down_wanted(int cin, int cout, int r_cout, int h, int w, int B, int mode) {
    if (mode >= 2) return true;
    if (mode <= 0) return false;
    const long px = (long)B * h * w;
    if (cin == 108 && cout == 46 && r_cout == 96) return px >= 131072 && px <= 1048576;
    return cin == 76 && cout == 28 && r_cout == 64 && px >= 524288 && px <= 4194304;
}

// conv_s4.hip lo (a three-tile 3x3 conv's launch also computes the low-resolution half of the commuted upsample + 1x1 conv behind it)
// instead of the two launches?  mode = plan option fold_lo: 0 never, 2 wherever the form exists (tests, A/B runs), 1 (default): only the
// class of launches whose folded runs MEASURED faster than the two launches in every run (MI355X, 1024x2048 network, same box, the
// options 0 / 2 alternated three times: profiles/r10_experiments.md): 163 -> 46 -> 63 at 128x256, B = 4 .. 32 - 78-79 -> 64-65 us,
// 138 -> 108-111 us, 243-252 -> 200-203 us, 475-477 -> 388-392 us: the slice is not stored either.  Nothing else was measured
bool lo_wanted(int cin, int cout, int r_cout, int h, int w, int B, int mode) {
    if (mode >= 2) return true;
    if (mode <= 0) return false;
    const long px = (long)B * h * w;
    return cin == 163 && cout == 46 && r_cout == 63 && px >= 131072 && px <= 1048576;
}

ConvChoice choose_conv(int ks, int stride, int cin, int cout, int hout, int wout, int B, int need, int use_tuned) {
    if (stride != 1) return ConvChoice::dma();           // shape by its cost model
    // The table was measured at B = 1, 2, 4, 8, 16 and (round 5, the strict-fp32 model at the headline's sub-batch) 32; a layer
    // without a row at one of those: the heuristics below won there.  Any other batch size takes the decision of the nearest
    // measured one (in ratio; the larger on a tie; beyond the largest: the largest): the choice depends on how many tiles the
    // launch has, which moves slowly with B.
    int Bt = B, ht = hout, wt = wout;
    if (use_tuned) {
        // (a layer at another image size than the measured one: the batch at which the measured launch had as many pixels)
        double b_eq = (double)B;
        bool exact = true;
        if (!measured_geometry(ks, cin, cout, hout, wout, B, &ht, &wt, &b_eq, &exact)) { ht = hout; wt = wout; b_eq = (double)B; }
        const int measured[6] = {1, 2, 4, 8, 16, 32};
        Bt = measured[5];
        for (int m : measured)
            if ((double)m >= b_eq) { Bt = (m > 1 && (double)m != b_eq && b_eq * b_eq < (double)m * (m / 2)) ? m / 2 : m; break; }
    }
    // (a layer without a B = 32 row: the cost model / heuristics below measured faster there - rows are kept only where they win by
    //  > 3 % - so it does NOT fall back to its B = 16 row)
    for (const Tuned &t : kTuned)
        if (use_tuned && t.ks == ks && t.cin == cin && t.cout == cout && t.hout == ht && t.wout == wt && t.B == Bt &&
            (!(need & 2) || !t.c.is(CONV_WAVE) || t.c.wave_mh() != 1))
            return t.c;
    // Untuned shape.  Large stride-1 3x3 layers go to the split kernel: on every measured shape with >= 64x128
    // pixels x 4 images it beat the fp32-MFMA kernels by 1.3-2.2x (profiles/README.md); cout tiles per workgroup by
    // channel count, 8x64 tiles where the image is wide enough to still fill the chip.  (The schedule gives the layer to
    // conv_dma when it needs a fused epilogue or split_f16 is off, hardnet_plan.hip.)
    if (ks == 3 && (need == 0) && (wout & 3) == 0 && (long)B * hout * wout >= 32768) {
        const int nt = cout <= 16 ? 1 : (cout <= 32 ? 2 : 3);
        const long tiles_wide = (long)B * ((hout + 7) / 8) * ((wout + 63) / 64) * (((cout + 15) / 16 + nt - 1) / nt);
        return ConvChoice::split(nt, (nt <= 2 && tiles_wide >= 512) ? 1 : 0);
    }
    // Images of >= 256x512 pixels keep the barrier-synchronised kernel (its big shared tiles move the
    // fewest bytes); below that the wave-autonomous kernel wins everywhere it was measured.  Pick the tile with the
    // most operand reuse (rows x cout tiles) that still puts >= 2 waves on every SIMD of the chip.
    // (1x1 layers from 32 768 pixels up too - round 5: at 512x1024, B = 16 the wave kernel took the 1x1 layers of the 32x64 level; it
    //  cannot write the packed-pair layout, so every 3x3 layer of that level fell back to the fp32-source split kernel: 0.56 of
    //  2.76 ms.  The measured table of the 1024x2048 network makes the same cut: packed pairs down to 32x64 at B = 16.)
    const long px = (long)B * hout * wout;
    if (px >= 131072 || (ks == 1 && px >= 32768)) return ConvChoice::dma();
    const int ntiles = (cout + 15) / 16;
    ConvChoice best = ConvChoice::wave((need & 2) ? 2 : 1, 1, 8);
    long best_reuse = -1, best_waves = -1;
    const int mhs[3] = {4, 2, 1}, wks[3] = {2, 4, 8};
    for (int mh : mhs)
        for (int nt = 2; nt >= 1; --nt) {
            if ((need & 2) && mh == 1) continue;
            if (nt > ntiles) continue;
            for (int wk : wks) {
                if (wave_lds_bytes(ks, mh, nt, wk) > 64 * 1024) continue;
                const long waves = (long)B * ((hout + mh - 1) / mh) * ((wout + 15) / 16) * ((ntiles + nt - 1) / nt) * wk;
                const long reuse = waves >= 2048 ? mh * nt : 0;
                if (reuse > best_reuse || (reuse == best_reuse && reuse == 0 && waves > best_waves)) {
                    best = ConvChoice::wave(mh, nt, wk);
                    best_reuse = reuse;
                    best_waves = waves;
                }
            }
        }
    return best;
}

S4Shape s4_resolve(int ks, int nt, int tile, int ntiles, int rounds, bool kacc) {
    nt = nt < 1 ? 1 : (nt > ntiles ? ntiles : nt);
    if (ks != 3) return {nt > 4 ? 4 : nt, 32, 8, 1};
    if (kacc) return {nt > 3 ? 3 : nt, 32, 8, 1};   // one workgroup per CU fewer than the plain form: 1 - 3 cout tiles
    const int nt2 = nt == 1 ? 1 : 2;
    if (tile == S4_16x32) return {nt2, 32, 16, 1};
    if (tile == S4_8x32_K4 && rounds >= 16) return {nt2, 32, 8, 4};   // (small images, long K)
    if (tile >= S4_8x32_K2 && rounds >= 8) return {nt2, 32, 8, 2};
    if (tile >= S4_8x32_K2 || tile == S4_8x32) return {nt > 4 ? 4 : nt, 32, 8, 1};   // too few rounds to split: plain 8x32
    if (nt <= 2) return {nt, 64, 8, 1};
    return {3, 32, 8, 1};   // 3 cout tiles: the 8x64 stages would leave one workgroup per CU
}

ConvChoice conv_force() { return g_conv_force; }

// pf_debug_force_conv in the inference schedule: (1, ..) and (2, ..) replace the fp32-source kernel of every conv (conv_wave: stride 1),
// (4, ..) where the plan has the split packing and the kernel the epilogue, (5, nt, tile) puts every eligible conv on conv_s4 with that shape
// and the others on conv_dma, which can write what those read
ConvDecision decide_conv(const ConvQuery &q) {
    const ConvChoice &f = q.force;
    const bool forced_s4 = f.is(CONV_S4), split_ok = q.has_split && (!q.need || q.ks == 1);
    ConvDecision d{{CONV_AUTO, 0, 0, 0}, false, 0, 0, {}};
    ConvChoice &ch = d.ch;
    if (!q.generic) {
        ch = choose_conv(q.ks, q.stride, q.cin, q.cout, q.hout, q.wout, q.B, q.need, q.use_tuned);
        if (f.is(CONV_WAVE) && q.stride == 1) ch = ConvChoice::wave((q.need & 2) && f.wave_mh() == 1 ? 2 : f.wave_mh(), f.wave_nt(), f.wave_wk());
        if (f.is(CONV_DMA) || (f.is(CONV_SPLIT) && split_ok)) ch = f;
        if (forced_s4 || (ch.is(CONV_SPLIT) && !(split_ok && q.split_f16))) ch = ConvChoice::dma();
    }
    // reads S4: the layers the table gives to the split kernels (same tile parameters), big 1x1 convs, all under a forced conv_s4 -
    // unless the measured conv_s4 row of the layer decides, and names the shape
    const bool split = ch.is(CONV_SPLIT);
    bool want = split || (q.ks == 1 && (long)q.B * q.hout * q.wout >= 32768 && ch.is(CONV_DMA)) || forced_s4;
    d.s4_nt = forced_s4 ? f.s4_nt() : (q.ks == 1 ? 4 : (split ? ch.split_nt() : 2));
    d.s4_tile = forced_s4 ? f.s4_tile() : (split ? ch.split_wide() : S4_8x32);
    ConvChoice row;
    if (!forced_s4 && !q.generic && q.use_tuned && choose_s4(q.ks, q.cin, q.cout, q.hout, q.wout, q.B, &row)) {
        want = row.is(CONV_S4);
        if (want) { d.s4_nt = row.s4_nt(); d.s4_tile = row.s4_tile(); }
    }
    d.wants_s4 = want && (forced_s4 || f.is(CONV_AUTO)) && !q.generic && q.stride == 1 && q.has_s4 && (q.need == 0 || q.ks == 1);
    d.s4 = s4_resolve(q.ks, d.s4_nt, d.s4_tile, (q.cout + 15) / 16, q.rounds, q.kacc);
    return d;
}

}  // namespace pf

static long long *g_probe_dev = nullptr;
namespace pf {
long long *probe_buffer() {
    if (!g_probe_dev) {
        if (hipMalloc((void **)&g_probe_dev, 64 * sizeof(long long)) != hipSuccess) return nullptr;
        (void)hipMemset(g_probe_dev, 0, 64 * sizeof(long long));
        (void)hipMemset(g_probe_dev + 60, 0xFF, sizeof(long long));
    }
    return g_probe_dev;
}
}  // namespace pf

/* PF_PROBE builds: copy out the 64 in-kernel timestamps recorded by the last probed launch (synchronises). */
extern "C" int pf_debug_probe_read(long long *host64) {
    if (!g_probe_dev) return PF_EINVAL;
    if (hipMemcpy(host64, g_probe_dev, 64 * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return PF_EHIP;
    (void)hipMemset(g_probe_dev, 0, 64 * sizeof(long long));
    (void)hipMemset(g_probe_dev + 60, 0xFF, sizeof(long long));   // slot 60 is an atomicMin target
    return PF_OK;
}

extern "C" int pf_debug_force_conv(int kind, int p0, int p1, int p2) {
    pf::g_conv_force = pf::ConvChoice{kind, p0, p1, p2};
    return PF_OK;
}

extern "C" int pf_debug_conv_decision(int ks, int stride, int cin, int cout, int hout, int wout, int B, int need, int flags, int rounds,
                                      int *out, int cap) {
    if (!out || cap < 11) return pf::fail(PF_EINVAL, "pf_debug_conv_decision: 11 ints of output");
    const pf::ConvDecision d = pf::decide_conv({ks, stride, cin, cout, hout, wout, B, need, (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0,
                                                (flags & 8) != 0, (flags & 16) != 0, (flags & 32) != 0, rounds, pf::conv_force()});
    const int v[11] = {d.ch.kind, d.ch.p0, d.ch.p1, d.ch.p2, d.wants_s4, d.s4_nt, d.s4_tile, d.s4.NT, d.s4.TW, d.s4.TH, d.s4.KS};
    for (int i = 0; i < 11; ++i) out[i] = v[i];
    return PF_OK;
}
