// The 3x3 packed-pair kernel's definition, included by conv_s4.hip once per form (the text of the plain form's function is the same
// whichever other forms exist: no wrapper, no extra template parameter in its symbol):
//   S4_KERNEL_NAME   conv_s4_kernel | conv_s4_blocked_kernel
//   S4_KERNEL_KACC   0 | 1: every round's products summed on their own and added to a second accumulator set (training)
//   S4_KERNEL_WAVES  waves per SIMD of __launch_bounds__
//   S4_KERNEL_EPI    0 | 1 "share" | 2 "add": the epilogue (DESIGN.md 4; ConvArgs::share ..).  share: matrix rows from a.share_off on are
//                    ANOTHER conv's sums over this launch's source, stored as fp32 units of four channels (acc * a.share_scale; no bias,
//                    no ReLU, no range report); the rows below it take the plain epilogue.  add: v = fma(acc, acc_scale, stored) + bias
//                    3 "tail" | 4 "down": the folds (NT = 2; ConvArgs::fold_..).  This conv's slice is read last by a 1x1 conv R.  The finished
//                    values stay in registers as the two terms R would read back and are multiplied by R's weights together with the
//                    centre pixels of R's other channels, so R's launch goes away.
//                      tail (ConvArgs::tail_..): R has no ReLU and one cout tile; its output is stored (fp32 NCHW), this conv's slice is not
//                      down (8 x 32 tiles; ConvArgs::down_..): the slice IS stored, as by the plain epilogue; R has a ReLU and up to four
//                      cout tiles, and its 2x2 average pool - two M-tile rows of a wave, lane pairs of a row - is stored (packed pairs or
//                      fp32 NCHW)
//                    The wide forms (NT = 3): a lane's 4 values of the third cout tile are the low half of one more K slice of R (chunk 2; R's
//                    fragments hold zeros above them), three products more per M-tile and cout tile of R.  4 "down" again, R of up to six
//                    cout tiles; 5 "lo": R is the low-resolution half of a commuted upsample + 1x1 conv - no bias, no ReLU, up to four
//                    cout tiles, stored as fp32 NCHW like tail's (ConvArgs::tail_..) - and the slice is stored unless a.dst is nullptr
template <int NT, int TW_, int TH_, int KS_>
__global__ __launch_bounds__(32 * TH_ * KS_, S4_KERNEL_WAVES) void S4_KERNEL_NAME(ConvArgs a) {
    [[maybe_unused]] constexpr int KACC = S4_KERNEL_KACC;
    [[maybe_unused]] constexpr int EPI = S4_KERNEL_EPI;
#if defined(__HIP_DEVICE_COMPILE__)
    using C = S4Cfg<NT, TW_, TH_, KS_>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
    const int lane = threadIdx.x & 63;
    const int wave_all = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int kgrp = C::KS > 1 ? wave_all / C::NW : 0;            // wave group of the K split (uniform)
    const int wave = C::KS > 1 ? wave_all % C::NW : wave_all;      // wave inside its group
    const int tid = C::KS > 1 ? (int)threadIdx.x & (C::NTHR - 1) : (int)threadIdx.x;   // thread inside its group
    unsigned char *const smem_raw = smem_all + kgrp * C::STAGES_BYTES;   // this group's stage ring
    int tid_lin, cgroup;   // XCD-aware order of tiles and cout groups (conv_mfma.h)
    xcd_tile_order(a.tilesX * a.tilesY, tid_lin, cgroup);
    const int tileY = tid_lin / a.tilesX, tileX = tid_lin - tileY * a.tilesX;
    const int tile0 = cgroup * NT, b = blockIdx.z;
    const int iy0 = tileY * C::TH - 1, ix0 = tileX * C::TW - 2;
    const size_t plane_bytes = (size_t)a.Hin * a.Win * 8;
    auto abuf = [&](int i) { return smem_raw + i * C::ABUF; };
    auto wbuf = [&](int i) { return smem_raw + 2 * C::ABUF + i * C::WBUF; };

    s4_f32x4 acc[C::MP][NT];
    [[maybe_unused]] s4_f32x4 tot[KACC ? C::MP : 1][KACC ? NT : 1];
#pragma unroll
    for (int m = 0; m < C::MP; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            acc[m][n] = s4_f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (KACC) tot[m][n] = s4_f32x4{0.f, 0.f, 0.f, 0.f};
        }

    // this lane's pieces of the plane its wave fetches: byte offset inside a group plane, or out of range
    // this wave's plane of a stage and its first DMA instruction of that plane (4 waves: one plane each, all of it)
    const int w4 = C::NW == 4 ? wave : (wave & 3), jb = C::NW == 4 ? 0 : (wave >> 2) * C::NDMA;
    unsigned poff[C::NDMA];
#pragma unroll
    for (int j = 0; j < C::NDMA; ++j) {
        const int p = (jb + j) * 64 + lane, row = p / C::ROWP, cp = p - row * C::ROWP;
        const int gy = iy0 + row, gx = ix0 + 2 * cp;
        poff[j] = (p < C::PIECES && gy >= 0 && gy < a.Hin && gx >= 0 && gx < a.Win) ? (unsigned)(gy * a.Win + gx) * 8u : kS4Oob;
    }
    // weight pieces of a stage: piece p -> (cout tile n, block, [term][lane]); the same byte offset in LDS and, per tile, in
    // the packed stream (blocks of a round are consecutive there)
    const int nblocks = s4_blocks_total(a.nchunks);
    unsigned woff[C::NITW];
    bool wcol[C::NITW];                    // piece of the collected-tap block (BPT = 3 only): fetched in flush rounds only
#pragma unroll
    for (int it = 0; it < C::NITW; ++it) {
        const int p = it * C::NTHR + tid, n = p / (C::BPT * 2 * 64), rem = p - n * (C::BPT * 2 * 64);
        woff[it] = (p < C::WPIECES && tile0 + n < a.ntiles) ? ((unsigned)(tile0 + n) * (unsigned)nblocks * (2 * 64) + (unsigned)rem) * 16u : kS4Oob;
        wcol[it] = rem >= 2 * 2 * 64;
    }
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.wpk, 0, 0x7FFFFFFF, 0x00020000);

    // A-fragment byte offsets inside a plane (M-tile part added as an immediate): the lane group picks the tap of instr 0 / 1;
    // the collected tap (2,2) is the same for every lane
    const int g = lane >> 4;
    int aoff[2], aoff_col;
    {
        const int ky[2] = {g >> 1, g < 2 ? 2 : g - 2};
        const int kx[2] = {g & 1, g < 2 ? g : 2};
        // (M-tile = 16 consecutive pixels of a row.  Pairing even / odd pixels for 16-B epilogue stores was built and measured
        //  +12 % on the fragment reads: profiles/r03_experiments.md)
#pragma unroll
        for (int s = 0; s < 2; ++s) aoff[s] = ((wave * 2 + ky[s]) * C::IW + (lane & 15) + kx[s] + 1) * 8;
        aoff_col = ((wave * 2 + 2) * C::IW + (lane & 15) + 2 + 1) * 8;
    }

    // operand roles are swapped with respect to conv_split.hip (weights = A, pixels = B): the D fragment of lane (g, i) is
    // couts 4g .. 4g+3 of a pixel = one 8-B unit of the packed layout per term, no cross-lane traffic in the epilogue.
    // The bias values of the workgroup's couts go to LDS by DMA now (4 B per lane, zero for couts past the layer) and are
    // read back in the epilogue: kept in registers across the main loop they cost NT * 4 registers (spilled at NT = 2, 3),
    // and either way the epilogue had to wait for them with vmcnt - which on gfx950 also waits for the epilogue's own stores
    float *bias_lds = reinterpret_cast<float *>(smem_all + C::KS * C::STAGES_BYTES);
    if (wave_all == 0 && lane < NT * 16) {
        const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc((void *)a.bias, 0, 0x7FFFFFFF, 0x00020000);
        const int co = tile0 * 16 + lane;
        // (share: the bias array is the odd layer's, padded to ITS tiles)
        const int nbias = EPI == 1 ? (a.Cout + 15) / 16 * 16 : a.ntiles * 16;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(brs, (s4_lds_ptr_t)bias_lds, 4, co < nbias ? (unsigned)co * 4u : kS4Oob, 0, 0, 0);
    }

    const int nrounds = a.nchunks;   // 3x3 launches always run the whole K range (the collected tap spans 4 rounds)
    // K split: group k runs rounds [k * chunk, (k + 1) * chunk); chunk is a multiple of 4, so every group but the last ends on a
    // flush round and all see whole groups of four collected-tap rounds.  All groups execute the same number of barriers
    const int chunk = C::KS > 1 ? (((nrounds + C::KS - 1) / C::KS + 3) / 4) * 4 : nrounds;
    const int r_begin = min(nrounds, kgrp * chunk), r_end = min(nrounds, r_begin + chunk);
    const int n_iter = chunk;
    // The DMA instructions of the next stage go out between the matrix groups of the current one (a part = one activation
    // piece + its share of the weight pieces): issued in one block they cost the wave ~1000 clocks per round in which it
    // feeds no MFMA (tools/probe_s4.py).
    constexpr int HALVES = C::MP / 4;
    __amdgpu_buffer_rsrc_t ars;
    unsigned asoff = 0;
    bool areal = true;
    auto prepare_round = [&](int r) {
        // activations: wave w fetches plane (term = w >> 1, entry = 2 r + (w & 1))
        const char *base;
        unsigned goff, tstride;
        areal = s4_entry(a, 2 * r + (w4 & 1), b, plane_bytes, base, goff, tstride);
        ars = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, 0x7FFFFFFF, 0x00020000);
        asoff = goff + (unsigned)(w4 >> 1) * tstride;
    };
    auto is_flush = [&](int r) { return (r & 3) == 3 || r == nrounds - 1; };
    auto issue_part = [&](int r, int stage, int j) {
        if ((jb + j) * 64 + lane < C::PIECES)   // the plane holds exactly its pieces: lanes past the last one write nothing
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ars, (s4_lds_ptr_t)(abuf(stage) + w4 * C::PLANE + (jb + j) * 1024), 16,
                                                     areal ? poff[j] : kS4Oob, asoff, 0, 0);
        unsigned char *wdst = wbuf(stage);
        const bool flush = is_flush(r);
#pragma unroll
        for (int it = j; it < C::NITW; it += C::NDMA)
            if (it * C::NTHR + tid < C::WPIECES && (flush || !wcol[it]))
                __builtin_amdgcn_raw_ptr_buffer_load_lds(wrsrc, (s4_lds_ptr_t)(wdst + (it * C::NTHR + wave * 64) * 16), 16, woff[it],
                                                         (unsigned)s4_blocks_before(r) * C::WBLK, 0, 0);
    };
    // part j of the next stage goes out after MFMA group kS4IssueFirst + j * kS4IssueStep of the round (6 HALVES groups)
    auto issue_slot = [&](int round, bool more, int slot) {
        if (!more) return;
#pragma unroll
        for (int j = 0; j < C::NDMA; ++j)
            if (slot == kS4IssueFirst + j * kS4IssueStep) issue_part(round + 1, (round + 1) & 1, j);
    };
    static_assert(kS4IssueFirst + (C::NDMA - 1) * kS4IssueStep < 6 * HALVES, "every DMA part needs a slot inside the two full instructions");   // (batches of 2 M-tiles: 12 slots)

    // collected tap: K-slice g of these fragments = entries of round 4q + g
    s4_h8 col_h[C::MP], col_m[C::MP];
    const s4_h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int m = 0; m < C::MP; ++m) col_h[m] = col_m[m] = zero8;

    if (r_begin < r_end) {
        prepare_round(r_begin);
#pragma unroll
        for (int j = 0; j < C::NDMA; ++j) issue_part(r_begin, r_begin & 1, j);
    }
    for (int it_ = 0; it_ < n_iter; ++it_) {
        const int round = r_begin + it_;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of the stage have landed
        S4_PROBE(round * 4 + 0);
        __syncthreads();                                    // everyone's have, and everyone is done reading the other stage
        S4_PROBE(round * 4 + 1);
        if (C::KS > 1 && round >= r_end) continue;          // a shorter part of a K split idles through the others' last rounds
        const bool more = round + 1 < r_end;
        if (more) prepare_round(round + 1);
        S4_PROBE(round * 4 + 2);
        const unsigned char *ab = abuf(round & 1), *wb = wbuf(round & 1);
        // Pixel fragments: a B operand is 8 fp16 = the 4 channels of TWO group entries of one pixel, which live in two planes of a
        // stage, 2880 B apart - out of reach of one ds_read2_b64 (255 x 8 B).  Left alone, hipcc pairs the reads of two DIFFERENT
        // M-tiles of one plane into a ds_read2_b64 and then moves the halves into place: 72 v_mov_b32 per round next to 54 matrix
        // instructions (and a ds_read2_b64 occupies the LDS for 8 cycles where two ds_read_b64 take 4).  Hence four plain
        // volatile ds_read_b64, each straight into its half of an operand tuple: no pairing, no moves
        auto frag = [&](const unsigned char *p, s4_h8 &h, s4_h8 &md) {
            typedef const volatile __attribute__((address_space(3))) s4_h4 *lds_h4;
            const lds_h4 q = (lds_h4)(const __attribute__((address_space(3))) unsigned char *)p;
            constexpr int PL = C::PLANE / 8;
            h = s4_join(q[0], q[PL]);
            md = s4_join(q[2 * PL], q[3 * PL]);
        };
        auto mtile_off = [&](int mm) {
            return ((mm / C::MTR) * C::IW + (mm % C::MTR) * 16) * 8;
        };
        // the three products of one block of weights with FT M-tiles; `slot0` numbers the MFMA groups for the DMA parts.
        // FT = 4 M-tiles per batch of fragment reads, or 2 for <2, 32>: its 126 registers have no room for 32 fragment registers
        // that are all live at once (the reads are volatile: none may be sunk below a matrix instruction) - two tiles at a time
        // need 16
        constexpr int FT = (NT == 2 && C::MP == 4) ? 2 : 4;
        auto mfmas = [&](const s4_h8 (&wh)[NT], const s4_h8 (&wm)[NT], int m0, const auto &fh, const auto &fm, int slot0, bool dma) {
            constexpr int FTn = (int)(sizeof(fh) / sizeof(fh[0]));
#pragma unroll
            for (int m = 0; m < FTn; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    acc[m0 + m][n] = PF_MFMA_SPLIT(wh[n], fm[m], acc[m0 + m][n]);
            if (dma) issue_slot(round, more, slot0 + 0);
#pragma unroll
            for (int m = 0; m < FTn; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    acc[m0 + m][n] = PF_MFMA_SPLIT(wm[n], fh[m], acc[m0 + m][n]);
            if (dma) issue_slot(round, more, slot0 + 1);
#pragma unroll
            for (int m = 0; m < FTn; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    acc[m0 + m][n] = PF_MFMA_SPLIT(wh[n], fh[m], acc[m0 + m][n]);
            if (dma) issue_slot(round, more, slot0 + 2);
        };
        constexpr int NB = C::MP / FT;      // fragment batches per instruction of a round
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            s4_h8 wh[NT], wm[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                wh[n] = *reinterpret_cast<const s4_h8 *>(wb + (((n * C::BPT + s) * 2 + 0) * 64 + lane) * 16);
                wm[n] = *reinterpret_cast<const s4_h8 *>(wb + (((n * C::BPT + s) * 2 + 1) * 64 + lane) * 16);
            }
#pragma unroll
            for (int bt = 0; bt < NB; ++bt) {
                s4_h8 fh[FT], fm[FT];
#pragma unroll
                for (int m = 0; m < FT; ++m) frag(ab + aoff[s] + mtile_off(bt * FT + m), fh[m], fm[m]);
                mfmas(wh, wm, bt * FT, fh, fm, 3 * (s * NB + bt), true);
                __builtin_amdgcn_sched_barrier(0);   // keep the next unit's fragment reads behind these MFMAs (registers)
            }
        }
        // the ninth tap of this round's entries: K-slice (round & 3)
        if (g == (round & 3)) {
#pragma unroll
            for (int m = 0; m < C::MP; ++m) frag(ab + aoff_col + mtile_off(m), col_h[m], col_m[m]);
        }
        if (is_flush(round)) {
            // the collected-tap block of this flush round (third block of the round in the packed stream).  COLREG: global ->
            // registers (L2-resident; the fragment registers of the two full instructions are dead here); else from LDS
            s4_h8 cwh[NT], cwm[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                if (C::COLREG) {
                    const bool real = tile0 + n < a.ntiles;   // uniform
                    const char *wp = reinterpret_cast<const char *>(a.wpk) +
                                     ((size_t)(real ? tile0 + n : 0) * nblocks + s4_blocks_before(round) + 2) * C::WBLK + lane * 16;
                    cwh[n] = real ? *reinterpret_cast<const s4_h8 *>(wp) : zero8;
                    cwm[n] = real ? *reinterpret_cast<const s4_h8 *>(wp + 64 * 16) : zero8;
                } else {
                    cwh[n] = *reinterpret_cast<const s4_h8 *>(wb + (((n * 3 + 2) * 2 + 0) * 64 + lane) * 16);
                    cwm[n] = *reinterpret_cast<const s4_h8 *>(wb + (((n * 3 + 2) * 2 + 1) * 64 + lane) * 16);
                }
            }
#pragma unroll
            for (int hf = 0; hf < HALVES; ++hf) {
                s4_h8 fh[4], fm[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    fh[m] = col_h[hf * 4 + m];
                    fm[m] = col_m[hf * 4 + m];
                }
                mfmas(cwh, cwm, hf * 4, fh, fm, 0, false);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int m = 0; m < C::MP; ++m) col_h[m] = col_m[m] = zero8;
        }
        if constexpr (KACC) {
#pragma unroll
            for (int m = 0; m < C::MP; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    tot[m][n] += acc[m][n];
                    acc[m][n] = s4_f32x4{0.f, 0.f, 0.f, 0.f};
                }
        }
        S4_PROBE(round * 4 + 3);
    }
    if constexpr (KACC) {
#pragma unroll
        for (int m = 0; m < C::MP; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = tot[m][n];
    }
    S4_PROBE(58);
    if (C::KS > 1) {
        // hand-over of the K split: groups 1.. park their sums in their own stage rings (conflict-free 16-B units), group 0 adds them
        __syncthreads();                                    // every wave is done reading its ring
        if (kgrp > 0) {
            s4_f32x4 *red = reinterpret_cast<s4_f32x4 *>(smem_raw);
#pragma unroll
            for (int m = 0; m < C::MP; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) red[((m * NT + n) * C::NW + wave) * 64 + lane] = acc[m][n];
        }
        __syncthreads();
        if (kgrp > 0) return;
#pragma unroll
        for (int k = 1; k < C::KS; ++k) {
            const s4_f32x4 *red = reinterpret_cast<const s4_f32x4 *>(smem_all + k * C::STAGES_BYTES);
#pragma unroll
            for (int m = 0; m < C::MP; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[m][n] += red[((m * NT + n) * C::NW + wave) * 64 + lane];
        }
    }

    // ---- epilogue: bias + ReLU; lane (g, i) holds couts 4g..4g+3 of the pixel pair (2i, 2i+1) of every M-tile pair: one
    //      16-B unit [2 px][4 ch] per term, or fp32 NCHW pairs
    {
        // Nothing in flight may be left for the compiler's wait-count pass to protect inside the store loop below: the main
        // loop's waits are inline asm (invisible to the pass), so a register it believes pending - a scratch reload, a value
        // loaded before the loop - got an s_waitcnt vmcnt(0) in EVERY iteration of that loop, and on gfx950 stores count in
        // vmcnt: each unit then sat through the store round trips of the unit before it (tools/asm_store_waits.py lists the
        // kernels that wait for their own stores).  One wait the pass can see, here:
        // (add: the lane's units of the stored sums are loaded in front of that wait - the main-loop state is dead, they take its registers)
        [[maybe_unused]] s4_f32x4 part[EPI == 2 ? C::MP : 1][EPI == 2 ? NT : 1];
        [[maybe_unused]] const size_t su_frame = EPI ? (size_t)((a.share_cout + 3) >> 2) * a.Hout * a.Wout : 0;   // 16-B units per frame of a.share
        if constexpr (EPI == 2) {
#pragma unroll
            for (int m = 0; m < C::MP; ++m) {
                const int mt = wave * C::MP + m;
                const int oy = tileY * C::TH + mt / C::MTR;
                const int ox = tileX * C::TW + (mt % C::MTR) * 16 + (lane & 15);
                const bool in = oy < a.Hout && ox < a.Wout;
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const int co = (tile0 + n) * 16 + 4 * (lane >> 4);
                    part[m][n] = s4_f32x4{0.f, 0.f, 0.f, 0.f};
                    if (in && co < a.share_cout)
                        part[m][n] = reinterpret_cast<const s4_f32x4 *>(a.share)[(size_t)b * su_frame + (size_t)(co >> 2) * a.Hout * a.Wout +
                                                                                 (size_t)oy * a.Wout + ox];
                }
            }
        }
        // tail / down: the second conv R's operands that do not come out of this launch's accumulators, loaded in front of the same wait.
        // tail: its A fragments (one 16-row tile, two terms, chunk 0 = R's other channels, chunk 1 = this launch's couts; L2-resident) and
        // bias.  down: R has up to four cout tiles - 16 KB of fragments, too many to hold - so they and R's bias go by LDS-DMA into the
        // stage ring, which is dead once every wave has left the main loop, and are read back per cout tile (no load, hence no vmcnt
        // wait, between the stores below).  Both: the lane's B fragments of chunk 0 - lane group g supplies group entries 2g and 2g + 1
        // of R's other channels at the CENTRE pixel of every M-tile, straight from the packed planes (entries past the range, pixels
        // outside the image: the zero page)
        constexpr bool FOLD = EPI == 3 || EPI == 4 || EPI == 5;
        constexpr bool RING = EPI == 4 || EPI == 5;   // R's fragments pass through the stage ring, [cout tile][chunk NT][term][lane]
        [[maybe_unused]] constexpr int FRAG_BYTES = NT == 3 ? kWideFragBytes : kDownFragBytes, RTILES = NT == 3 ? kWideTiles : kDownTiles;
        [[maybe_unused]] s4_h8 tw_h[EPI == 3 ? 2 : 1], tw_m[EPI == 3 ? 2 : 1];
        [[maybe_unused]] s4_h4 to_h[FOLD ? C::MP : 1][2], to_m[FOLD ? C::MP : 1][2];
        [[maybe_unused]] s4_f32x4 tbias = s4_f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (EPI == 3) {
            static_assert(NT == 2, "a lane's 4 + 4 split values of two cout tiles are one K slice of the second conv");
            const s4_h8 *tw = reinterpret_cast<const s4_h8 *>(a.fold_w);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                tw_h[c] = tw[(c * 2 + 0) * 64 + lane];
                tw_m[c] = tw[(c * 2 + 1) * 64 + lane];
            }
            tbias = *reinterpret_cast<const s4_f32x4 *>(a.fold_bias + 4 * (lane >> 4));
        }
        if constexpr (RING) {
            static_assert((NT == 2 || NT == 3) && TW_ == 32 && TH_ == 8 && KS_ == 1, "M-tiles m and m + 2 of a wave are two rows of the same 16 columns");
            static_assert(NT == 3 || EPI == 4, "lo is built for three cout tiles");
            static_assert(FRAG_BYTES + RTILES * 16 * sizeof(float) <= C::STAGES_BYTES, "R's fragments and bias live in the stage ring");
            const int rt = (a.fold_cout + 15) >> 4;             // R's cout tiles (uniform)
            __syncthreads();                                    // every wave is done reading the ring
            const __amdgpu_buffer_rsrc_t frs = __builtin_amdgcn_make_buffer_rsrc((void *)a.fold_w, 0, 0x7FFFFFFF, 0x00020000);
#pragma unroll
            for (int it = 0; it < FRAG_BYTES / 16 / C::NTHR; ++it) {
                const int p = it * C::NTHR + tid;               // 16-B piece; a cout tile is NT * 128 of them
                __builtin_amdgcn_raw_ptr_buffer_load_lds(frs, (s4_lds_ptr_t)(smem_all + (it * C::NTHR + wave * 64) * 16), 16,
                                                         p < rt * (NT * 128) ? (unsigned)p * 16u : kS4Oob, 0, 0, 0);
            }
            if (wave < (RTILES * 16 + 63) / 64) {               // R's bias: 64 values per wave, zero past its tiles
                const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc((void *)a.fold_bias, 0, 0x7FFFFFFF, 0x00020000);
                const int bi = wave * 64 + lane;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(brs, (s4_lds_ptr_t)(smem_all + FRAG_BYTES + wave * 256), 4, bi < rt * 16 ? (unsigned)bi * 4u : kS4Oob,
                                                         0, 0, 0);
            }
        }
        if constexpr (FOLD) {
            const size_t tstride = (size_t)a.fold_c4 * plane_bytes;
            const char *tbase = reinterpret_cast<const char *>(a.fold_src) + (size_t)b * 2 * tstride;
#pragma unroll
            for (int m = 0; m < C::MP; ++m) {
                const int mt = wave * C::MP + m;
                const int oy = tileY * C::TH + mt / C::MTR;
                const int ox = tileX * C::TW + (mt % C::MTR) * 16 + (lane & 15);
                const bool in = oy < a.Hout && ox < a.Wout;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int e = 2 * (lane >> 4) + h;
                    const bool real = in && e < a.fold_gn;
                    const char *p = real ? tbase + (size_t)(a.fold_g0 + e) * plane_bytes + ((size_t)oy * a.Wout + ox) * 8
                                         : reinterpret_cast<const char *>(a.zero_page);
                    to_h[m][h] = *reinterpret_cast<const s4_h4 *>(p);
                    to_m[m][h] = *reinterpret_cast<const s4_h4 *>(real ? p + tstride : p);
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);        // vmcnt(0), expcnt / lgkmcnt untouched
        if constexpr (RING) __syncthreads();       // every wave's pieces of R's fragments have landed
        const int g = lane >> 4, px = lane & 15;
        const size_t hw = (size_t)a.Hout * a.Wout;
        const S4Dst sd = s4_dst(a, b, hw);         // this conv's slice (conv_epilogue.h: s4_store_px)
        const float relu_lo = a.relu ? 0.f : -__builtin_inff();
        float vmax = 0.f;                          // range guard of the operand split (conv_mfma.h)
        // folds: R's chunk 0 operand of M-tile m, the centre pixels of its other channels (K slice g: group entries 2g, 2g + 1)
        [[maybe_unused]] auto fold_chunk0 = [&](int m, s4_h8 &x0h, s4_h8 &x0m) {
            x0h = s4_join(to_h[m][0], to_h[m][1]); x0m = s4_join(to_m[m][0], to_m[m][1]);
        };
        // ... and R's sum for one M-tile and one of its cout tiles: chunk 0 (its other channels), then chunk 1 (this launch's), three
        // products each, one fp32 accumulator
        [[maybe_unused]] auto fold_products = [](const s4_h8 &wh0, const s4_h8 &wm0, const s4_h8 &wh1, const s4_h8 &wm1, const s4_h8 &x0h, const s4_h8 &x0m,
                                                 const s4_h8 &x1h, const s4_h8 &x1m) {
            s4_f32x4 t = s4_f32x4{0.f, 0.f, 0.f, 0.f};
            t = PF_MFMA_SPLIT(wh0, x0m, t);
            t = PF_MFMA_SPLIT(wm0, x0h, t);
            t = PF_MFMA_SPLIT(wh0, x0h, t);
            t = PF_MFMA_SPLIT(wh1, x1m, t);
            t = PF_MFMA_SPLIT(wm1, x1h, t);
            t = PF_MFMA_SPLIT(wh1, x1h, t);
            return t;
        };
        [[maybe_unused]] s4_h8 dx0h[RING ? C::MP : 1], dx0m[RING ? C::MP : 1], dx1h[RING ? C::MP : 1], dx1m[RING ? C::MP : 1];
        [[maybe_unused]] s4_h4 dx2h[RING && NT == 3 ? C::MP : 1], dx2m[RING && NT == 3 ? C::MP : 1];   // chunk 2: the third cout tile's values
        // ... and chunk 2's three products on top (wide forms)
        [[maybe_unused]] auto fold_products2 = [](s4_f32x4 t, const s4_h8 &wh2, const s4_h8 &wm2, const s4_h4 &x2h, const s4_h4 &x2m) {
            const s4_h4 zero4 = {0, 0, 0, 0};
            const s4_h8 xh = s4_join(x2h, zero4), xm = s4_join(x2m, zero4);
            t = PF_MFMA_SPLIT(wh2, xm, t);
            t = PF_MFMA_SPLIT(wm2, xh, t);
            t = PF_MFMA_SPLIT(wh2, xh, t);
            return t;
        };
        [[maybe_unused]] const bool slice_stored = EPI != 5 || a.dst != nullptr;   // (uniform)
#pragma unroll
        for (int m = 0; m < C::MP; ++m) {
            const int mt = wave * C::MP + m;
            const int oy = tileY * C::TH + mt / C::MTR;
            const int ox = tileX * C::TW + (mt % C::MTR) * 16 + px;
            if constexpr (EPI == 3) {
                // this launch's values as the plain epilogue would store them (rows past its couts: zero weights, zero bias -> 0), split
                // into the two terms R would read back; the lane's 4 + 4 values of the two cout tiles are K slice g of R's chunk 1 (the
                // packer's order: conv_ranges.cpp tail_channel).  Every lane takes part in the matrix instructions; lanes whose pixel
                // lies outside the image report nothing to the range guard and store nothing
                const bool in = oy < a.Hout && ox < a.Wout;
                s4_h4 xh[2], xm[2];
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const s4_f32x4 b4 = *reinterpret_cast<const s4_f32x4 *>(bias_lds + n * 16 + 4 * g);
                    const s4_f32x4 v = s4_finish(acc[m][n], a.acc_scale, b4, relu_lo);
                    const float vm = range_acc(vmax, v[0], v[1], v[2], v[3]);
                    vmax = in ? vm : vmax;
                    split_terms4(v, xh[n], xm[n]);
                }
                const s4_h8 x1h = s4_join(xh[0], xh[1]), x1m = s4_join(xm[0], xm[1]);
                s4_h8 x0h, x0m;
                fold_chunk0(m, x0h, x0m);
                const s4_f32x4 t = fold_products(tw_h[0], tw_m[0], tw_h[1], tw_m[1], x0h, x0m, x1h, x1m);
                if (in) {
                    const size_t pix = (size_t)oy * a.Wout + ox;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (4 * g + r < a.fold_cout)
                            a.tail_dst[((size_t)b * a.tail_ctotal + a.tail_choff + 4 * g + r) * hw + pix] = t[r] * a.fold_scale + tbias[r];
                }
                continue;
            }
            if constexpr (RING) {
                // the plain epilogue for every lane (rows past this launch's couts: zero weights, zero bias -> 0), the slice stored as the
                // plain form stores it; the same values split into the two terms R would read back are K slice g of R's chunk 1, as in
                // the tail form, and are kept for all four M-tiles next to chunk 0's
                const bool in = oy < a.Hout && ox < a.Wout;
                s4_h4 xh[NT], xm[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const int co = (tile0 + n) * 16 + 4 * g;
                    const s4_f32x4 b4 = *reinterpret_cast<const s4_f32x4 *>(bias_lds + n * 16 + 4 * g);
                    const s4_f32x4 v = s4_finish(acc[m][n], a.acc_scale, b4, relu_lo);
                    const float vm = range_acc(vmax, v[0], v[1], v[2], v[3]);
                    vmax = in ? vm : vmax;
                    split_terms4(v, xh[n], xm[n]);
                    if (in && co < a.Cout + 2 && slice_stored) s4_store_px(sd, co, (size_t)oy * a.Wout + ox, v);
                }
                dx1h[m] = s4_join(xh[0], xh[1]); dx1m[m] = s4_join(xm[0], xm[1]);
                if constexpr (NT == 3) { dx2h[m] = xh[2]; dx2m[m] = xm[2]; }
                fold_chunk0(m, dx0h[m], dx0m[m]);
                continue;
            }
            if (oy >= a.Hout || ox >= a.Wout) continue;
            const size_t pix = (size_t)oy * a.Wout + ox;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int co = (tile0 + n) * 16 + 4 * g;
                if constexpr (EPI == 1) {
                    // the consumer's rows: channels cs .. cs + 3 of its sums over this source, one fp32 unit (rows past its couts
                    // inside the last unit multiplied zero weights).  Not stored values of any tensor: no range_acc
                    const int cs = co - a.share_off;
                    if (cs >= 0) {
                        if (cs < a.share_cout) {
                            s4_f32x4 u = acc[m][n];
#pragma unroll
                            for (int r = 0; r < 4; ++r) u[r] *= a.share_scale;   // 2^-k: exact
                            reinterpret_cast<s4_f32x4 *>(a.share)[(size_t)b * su_frame + (size_t)(cs >> 2) * hw + pix] = u;
                        }
                        continue;
                    }
                }
                if (co >= a.Cout + 2) continue;
                s4_f32x4 v = acc[m][n];
                const s4_f32x4 b4 = *reinterpret_cast<const s4_f32x4 *>(bias_lds + n * 16 + 4 * g);
                if constexpr (EPI == 2) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = fmaxf(__builtin_fmaf(v[r], a.acc_scale, part[m][n][r]) + b4[r], relu_lo);
                } else {
                    v = s4_finish(v, a.acc_scale, b4, relu_lo);
                }
                vmax = range_acc(vmax, v[0], v[1], v[2], v[3]);
                if (a.dst_fmt) {
                    s4_store_px(sd, co, pix, v);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (co + r < a.Cout) a.dst[((size_t)b * a.dst_ctotal + a.dst_choff + co + r) * hw + pix] = v[r];
                }
            }
        }
        if constexpr (EPI == 4) {
            // R, one cout tile at a time: fold_products per M-tile, then 2^-k, bias, ReLU (R has one: plan_create.hip is_conv_down) and the 2x2 average pool in
            // registers.  M-tiles 0, 1 are row 2w of the tile (columns 0-15, 16-31), M-tiles 2, 3 row 2w + 1; the horizontal neighbour
            // sits in lane px ^ 1.  Even lanes pool M-tiles 0 / 2, odd lanes M-tiles 1 / 3: a lane sends its neighbour the value of the
            // tile the neighbour pools, so the 16 lanes of a lane group store 16 consecutive pooled pixels, 128 B per term.
            // (((a + b) + c) + d) * 0.25, a, b = row oy at x, x + 1: the order of avgpool2_kernel and conv_s4_1x1_kernel
            const int rt = (a.fold_cout + 15) >> 4;
            const int Ho = a.Hout >> 1, Wo = a.Wout >> 1;       // a last row or column the pool drops is not stored
            const size_t hw2 = (size_t)Ho * Wo, term2 = (size_t)a.down_c4 * hw2 * 8;
            const S4Dst dd = {reinterpret_cast<char *>(a.down_dst) + (size_t)b * 2 * term2, term2, hw2, a.down_choff, a.down_limit};   // R's (down_fmt)
            const bool odd = (px & 1) != 0;
            const int poy = tileY * (C::TH / 2) + wave, pox = tileX * (C::TW / 2) + (odd ? 8 : 0) + (px >> 1);
            const bool pin = poy < Ho && pox < Wo;
            const size_t ppix = (size_t)poy * Wo + pox;
            const unsigned char *fw = smem_all + lane * 16;
            const float *rbias = reinterpret_cast<const float *>(smem_all + FRAG_BYTES);
            float vmax2 = 0.f;
            auto swap_px = [](float x) {                         // the value of lane px ^ 1: quad_perm [1, 0, 3, 2]
                return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true));
            };
#pragma unroll 1
            for (int ct = 0; ct < rt; ++ct) {
                const s4_h8 wh0 = *reinterpret_cast<const s4_h8 *>(fw + (ct * 2 * NT + 0) * 1024), wm0 = *reinterpret_cast<const s4_h8 *>(fw + (ct * 2 * NT + 1) * 1024);
                const s4_h8 wh1 = *reinterpret_cast<const s4_h8 *>(fw + (ct * 2 * NT + 2) * 1024), wm1 = *reinterpret_cast<const s4_h8 *>(fw + (ct * 2 * NT + 3) * 1024);
                [[maybe_unused]] s4_h8 wh2, wm2;
                if constexpr (NT == 3) {
                    wh2 = *reinterpret_cast<const s4_h8 *>(fw + (ct * 6 + 4) * 1024); wm2 = *reinterpret_cast<const s4_h8 *>(fw + (ct * 6 + 5) * 1024);
                }
                const s4_f32x4 b4 = *reinterpret_cast<const s4_f32x4 *>(rbias + ct * 16 + 4 * g);
                s4_f32x4 v[C::MP];
#pragma unroll
                for (int m = 0; m < C::MP; ++m) {
                    s4_f32x4 t = fold_products(wh0, wm0, wh1, wm1, dx0h[m], dx0m[m], dx1h[m], dx1m[m]);
                    if constexpr (NT == 3) t = fold_products2(t, wh2, wm2, dx2h[m], dx2m[m]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[m][r] = fmaxf(t[r] * a.fold_scale + b4[r], 0.f);
                }
                s4_f32x4 pv;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float top = swap_px(odd ? v[0][r] : v[1][r]), bot = swap_px(odd ? v[2][r] : v[3][r]);
                    const float pa = odd ? top : v[0][r], pb = odd ? v[1][r] : top, pc = odd ? bot : v[2][r], pd = odd ? v[3][r] : bot;
                    pv[r] = (((pa + pb) + pc) + pd) * 0.25f;
                }
                const float vm = range_acc(vmax2, pv[0], pv[1], pv[2], pv[3]);
                vmax2 = pin ? vm : vmax2;
                const int co = ct * 16 + 4 * g;
                if (pin && !a.down_fmt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (co + r < a.fold_cout) reinterpret_cast<float *>(a.down_dst)[((size_t)b * a.down_ctotal + a.down_choff + co + r) * hw2 + ppix] = pv[r];
                } else if (pin && co < a.fold_cout + 2) {
                    s4_store_px(dd, co, ppix, pv);
                }
            }
            range_commit(a.down_status, a.down_slot, vmax2);
        }
        if constexpr (EPI == 5) {
            // R, one cout tile at a time, as in the down form; its values go out as the tail form's do: fp32 NCHW, 2^-k and bias (the zero
            // page: the other half of the commuted pair adds R's) and nothing else - the scratch is no operand of a split kernel
            const int rt = (a.fold_cout + 15) >> 4;
            const unsigned char *fw = smem_all + lane * 16;
            const float *rbias = reinterpret_cast<const float *>(smem_all + FRAG_BYTES);
#pragma unroll 1
            for (int ct = 0; ct < rt; ++ct) {
                const s4_h8 wh0 = *reinterpret_cast<const s4_h8 *>(fw + (ct * 6 + 0) * 1024), wm0 = *reinterpret_cast<const s4_h8 *>(fw + (ct * 6 + 1) * 1024);
                const s4_h8 wh1 = *reinterpret_cast<const s4_h8 *>(fw + (ct * 6 + 2) * 1024), wm1 = *reinterpret_cast<const s4_h8 *>(fw + (ct * 6 + 3) * 1024);
                const s4_h8 wh2 = *reinterpret_cast<const s4_h8 *>(fw + (ct * 6 + 4) * 1024), wm2 = *reinterpret_cast<const s4_h8 *>(fw + (ct * 6 + 5) * 1024);
                const s4_f32x4 b4 = *reinterpret_cast<const s4_f32x4 *>(rbias + ct * 16 + 4 * g);
                const int co = ct * 16 + 4 * g;
#pragma unroll
                for (int m = 0; m < C::MP; ++m) {
                    const int mt = wave * C::MP + m;
                    const int oy = tileY * C::TH + mt / C::MTR;
                    const int ox = tileX * C::TW + (mt % C::MTR) * 16 + px;
                    s4_f32x4 t = fold_products(wh0, wm0, wh1, wm1, dx0h[m], dx0m[m], dx1h[m], dx1m[m]);
                    t = fold_products2(t, wh2, wm2, dx2h[m], dx2m[m]);
                    if (oy < a.Hout && ox < a.Wout) {
                        const size_t pix = (size_t)oy * a.Wout + ox;
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (co + r < a.fold_cout)
                                a.tail_dst[((size_t)b * a.tail_ctotal + a.tail_choff + co + r) * hw + pix] = t[r] * a.fold_scale + b4[r];
                    }
                }
            }
        }
        range_commit(a.status, a.range_slot, vmax);
    }
    S4_PROBE(59);
#endif
}

