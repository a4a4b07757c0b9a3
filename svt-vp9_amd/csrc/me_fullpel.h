/* me_fullpel.h -- exhaustive integer-sample search: the stand-alone SAD loop (eb_vp9_sad_loop_kernel) and full_pel_search_sb with its
 * 85 nested PU sums -- the table form (sad8 / sum16 / sum32 / argmin) for any area, the fused form for widths that are multiples of 8. */
#ifndef SVT_ME_FULLPEL_H
#define SVT_ME_FULLPEL_H
#include "me_types.h"

/* Generic exhaustive SAD search (= eb_vp9_sad_loop_kernel) over a window staged in LDS.
 * blk: block rows (already subsampled) in LDS, stride bstride, bw x bh.  win: LDS window whose row r holds
 * reference row (window_top + r) and column 0 = search x position 0; a search row y uses window rows
 * y + mul*j (j = block row; mul = 2 in every reference use).  Key = (sad << 32) | (y * sw + x).  bw multiple of 4 uses QSAD. */
SVT_DEV void ph_sad_search(const me_ctx_t *c, int tid, const uint8_t *blk, int bstride, int bw, int bh, const uint8_t *win,
                           int wstride, int sw, int sh, int mul) {
    int      ng   = (sw + 3) >> 2;
    uint64_t best = ~0ull;
    if ((bw & 3) == 0) {
        int nd = bw >> 2;
        for (int t = tid; t < ng * sh; t += SVT_NT) {
            int      y = t / ng, g = t - y * ng;
            uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
            for (int j = 0; j < bh; j++) {
                const uint32_t *wr  = (const uint32_t *)(win + (y + mul * j) * wstride + 4 * g);
                const uint32_t *br  = (const uint32_t *)(blk + j * bstride);
                uint64_t        acc = 0;
                uint32_t        lo  = wr[0];
                for (int i = 0; i < nd; i++) {
                    uint32_t hi = wr[i + 1];
                    acc         = svt_qsad(((uint64_t)hi << 32) | lo, br[i], acc);
                    lo          = hi;
                }
                a0 += (uint32_t)(acc & 0xffff); a1 += (uint32_t)((acc >> 16) & 0xffff);
                a2 += (uint32_t)((acc >> 32) & 0xffff); a3 += (uint32_t)(acc >> 48);
            }
            uint32_t a[4] = {a0, a1, a2, a3};
            for (int o = 0; o < 4; o++) {
                int x = 4 * g + o;
                if (x < sw) {
                    uint64_t k = ((uint64_t)a[o] << 32) | (uint32_t)(y * sw + x);
                    if (k < best) best = k;
                }
            }
        }
    } else {
        for (int t = tid; t < sw * sh; t += SVT_NT) {
            int      y = t / sw, x = t - y * sw;
            uint32_t s = 0;
            for (int j = 0; j < bh; j++)
                for (int i = 0; i < bw; i++) {
                    int a = blk[j * bstride + i], b = win[(y + mul * j) * wstride + x + i];
                    s += (uint32_t)(a > b ? a - b : b - a);
                }
            uint64_t k = ((uint64_t)s << 32) | (uint32_t)t;
            if (k < best) best = k;
        }
    }
    svt_wave_min_u64(&c->st->hme_key, best);
}

/* full-pel search tables.  All 85 PU SADs of a search position live in one row of ME_PU_STRIDE dwords indexed by
 * the PU's search-order index (0 = 64x64, 1..4 = 32x32, 5..20 = 16x16, 21..84 = 8x8; children of a block are the 4
 * consecutive entries 4*z .. 4*z+3 of the next level, i.e. nested z-order).  Entries 0..20 are dwords; the 64 8x8 SADs
 * (sub-sampled, < 2^16) follow as halfwords.  The odd stride keeps the per-position rows on different LDS banks. */
#define ME_PU_STRIDE 53

/* full-pel: sub-sampled 8x8 SADs of every (position, 8x8 block) of a chunk of search rows.
 * Task = (8x8 block b in raster order, 4-position group g, search row y).  Output U[pos][21 + z(b)]
 * (pos = y_local * sw + x).  tail columns (x >= w8) reproduce the reference's address bug
 * for 16x16 blocks 12 and 13 (Codec/EbMotionEstimation.c:855-856). */
SVT_DEV void ph_fullpel_sad8(const me_ctx_t *c, int tid, uint32_t *U, int sw, int y0, int ny, int w8) {
    int ng = (sw + 3) >> 2;
    int rs = c->L.region_stride;
    for (int t = tid; t < ng * ny * 64; t += SVT_NT) {
        int b = t & 63, q = t >> 6;
        int yl = q / ng, g = q - yl * ng;
        int bx = (b & 7) * 8, by = (b >> 3) * 8;
        int rbx = bx;
        if (4 * g >= w8) {
            /* 16x16 block (raster) containing b: z-order 12 -> raster 10 (x=32,y=32), 13 -> raster 11 (x=48,y=32) */
            if (by >= 32 && by < 48 && bx >= 32) rbx += 16;
        }
        const uint8_t *rp = c->region + ME_MUL(ME_RGN_GY + y0 + yl + by, rs) + ME_RGN_GX + 4 * g + rbx;
        const uint8_t *sp = c->src + by * ME_SB + bx;
        uint64_t       acc = 0;
        _Pragma("unroll") for (int r = 0; r < 4; r++) {
            const uint32_t *w = (const uint32_t *)(rp + 2 * r * rs);
            const uint32_t *s = (const uint32_t *)(sp + 2 * r * ME_SB);
            uint32_t        d0 = w[0], d1 = w[1], d2 = w[2];
            acc = svt_qsad(((uint64_t)d1 << 32) | d0, s[0], acc);
            acc = svt_qsad(((uint64_t)d2 << 32) | d1, s[1], acc);
        }
        uint16_t *u = (uint16_t *)(U + ME_MUL(ME_MUL(yl, sw) + 4 * g, ME_PU_STRIDE) + 21) + me_z8(b);
        _Pragma("unroll") for (int o = 0; o < 4; o++)
            if (4 * g + o < sw) u[o * 2 * ME_PU_STRIDE] = (uint16_t)(acc >> (16 * o));
    }
}

#ifndef SVT_HOST_EMU /* device only: the two lane layouts of the fused phase; the emulation runs ph_fullpel_fused's serial per-position form; pinned by tests/test_gpu_me.py::test_me_large_search_areas_full_pel_layouts (its widths that are multiples of 16: the 16x16-PU layout) */
/* The device form of ph_fullpel_fused (below).  The instruction stream of a group of 4 positions is written out: both dwords of
 * every QSAD operand are read as a pair (two ds_read2 per row instead of register moves; the lane's LDS offsets are opaque to the
 * compiler so that a group costs ONE add per operand stream and the rows are immediate offsets), a key is one v_lshl_or /
 * v_and_or and five keys meet in two v_min3, the 32x32 step adds 16-bit halves across the row without unpacking them first, and
 * the 64x64 step is eight in-place DPP adds: 56 vector instructions per group (87 before).  NG = 2 evaluates two groups per
 * iteration with independent accumulators: for the configurations whose LDS need leaves one or two waves per SIMD (64x64 search
 * areas) the phase is bound by the latency of its dependent chains, not by issue. */
SVT_DEV uint32_t me_min3(uint32_t a, uint32_t b, uint32_t c) { const uint32_t m = a < b ? a : b; return m < c ? m : c; }
/* RUN (with NG = 2): the two groups of an iteration are NEIGHBOURS in a search row -- a run of 8 positions -- and share their operand pairs:
 * group 0 takes the pairs at +0 and +4 of a window row, group 1 those at +4 and +8: three reads per row instead of four (the LDS, shared by
 * the CU's five workgroups, is as busy as the vector unit in this kernel) */
template <int NG, bool RUN = false> SVT_DEV void me_fullpel_fused_dev(const me_ctx_t *c, int tid, int sw, int sh) {
    const int rs = c->L.region_stride;
    const int z = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bx = ((z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4)) * 8, by = (((z >> 1) & 1) | ((z >> 2) & 2) | ((z >> 3) & 4)) * 8;
    uint32_t  s0[4], s1[4]; /* rows 0, 2, 4, 6 of the source block */
    _Pragma("unroll") for (int r = 0; r < 4; r++) {
        const uint32_t *s = (const uint32_t *)(c->src + (by + 2 * r) * ME_SB + bx);
        s0[r] = s[0]; s1[r] = s[1];
    }
    uint32_t ro0 = (uint32_t)(c->region - c->lds) + (uint32_t)(ME_MUL(ME_RGN_GY + by, rs) + ME_RGN_GX + bx), ro1 = ro0 + 4;
    __asm__("" : "+v"(ro0));
    __asm__("" : "+v"(ro1));
    uint32_t mhi = 0xffff0000u;
    __asm__("" : "+v"(mhi)); /* in a vector register: (x & mhi) | s is then ONE v_and_or_b32 (one scalar operand per instruction) */
    const int ng = RUN ? sw >> 3 : sw >> 2; /* RUN: runs per search row */
    static_assert(!RUN || NG == 2, "a run is two groups");
    uint32_t  b8 = 0xffffffffu, b16 = 0xffffffffu, b32 = 0xffffffffu, b64 = 0xffffffffu;
#define FP_DPP(v, ctrl) ((v) + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), 0xf, 0xf, false))
#define FP_KEYS(b, lo, hi, pos) do { \
        b = me_min3(b, ((lo) << 16) | (pos), ((lo) & mhi) | ((pos) + 1)); \
        b = me_min3(b, ((hi) << 16) | ((pos) + 2), ((hi) & mhi) | ((pos) + 3)); } while (0)
    /* group q = y * ng + g (wave-uniform; y by reciprocal multiplication on the scalar unit: the body stays one basic block); the
     * waves take the groups round-robin, NG consecutive rounds per iteration (a group past the end repeats the last one: the
     * minima do not change) */
    const uint32_t inv = me_magics.v[ng]; /* ng in [2, 31] */
    const int      nq = ME_MUL(ng, sh);
    for (int q0 = w; q0 < nq; q0 += RUN ? 4 : 4 * NG) {
        uint32_t pos[NG], lo[NG], hi[NG], a0[NG], a1[NG], a2[NG], a3[NG];
        if constexpr (RUN) {
            const int      y = inv ? (int)(((uint64_t)(uint32_t)q0 * inv) >> 32) : q0, g = 2 * (q0 - y * ng);
            const int      off = ME_MUL(y, rs) + 4 * g; /* wave-uniform */
            const uint8_t *rp = c->lds + (ro0 + (uint32_t)off), *rp1 = c->lds + (ro1 + (uint32_t)off);
            uint64_t       acc = 0, acc_b = 0;
            _Pragma("unroll") for (int r = 0; r < 4; r++) {
                const uint64_t p0 = *(const me_u64a4 *)(rp + 2 * r * rs), p1 = *(const me_u64a4 *)(rp1 + 2 * r * rs), p2 = *(const me_u64a4 *)(rp + 2 * r * rs + 8);
                acc = svt_qsad(p0, s0[r], acc);     acc = svt_qsad(p1, s1[r], acc);
                acc_b = svt_qsad(p1, s0[r], acc_b); acc_b = svt_qsad(p2, s1[r], acc_b);
            }
            pos[0] = (uint32_t)(ME_MUL(y, sw) + 4 * g); pos[NG - 1] = pos[0] + 4;
            lo[0] = (uint32_t)acc; hi[0] = (uint32_t)(acc >> 32); lo[NG - 1] = (uint32_t)acc_b; hi[NG - 1] = (uint32_t)(acc_b >> 32);
        } else
        _Pragma("unroll") for (int u = 0; u < NG; u++) {
            const int      q = q0 + 4 * u < nq ? q0 + 4 * u : q0;
            const int      y = (int)(((uint64_t)(uint32_t)q * inv) >> 32), g = q - y * ng;
            const int      off = ME_MUL(y, rs) + 4 * g; /* wave-uniform */
            const uint8_t *rp = c->lds + (ro0 + (uint32_t)off), *rp1 = c->lds + (ro1 + (uint32_t)off);
            uint64_t       acc = 0;
            _Pragma("unroll") for (int r = 0; r < 4; r++) {
                const uint64_t pa = *(const me_u64a4 *)(rp + 2 * r * rs), pb = *(const me_u64a4 *)(rp1 + 2 * r * rs);
                acc = svt_qsad(pa, s0[r], acc);
                acc = svt_qsad(pb, s1[r], acc);
            }
            pos[u] = (uint32_t)(ME_MUL(y, sw) + 4 * g);
            lo[u] = (uint32_t)acc; hi[u] = (uint32_t)(acc >> 32); /* positions pos, pos + 1 | pos + 2, pos + 3 as 16-bit sums */
        }
        _Pragma("unroll") for (int u = 0; u < NG; u++) {
            FP_KEYS(b8, lo[u], hi[u], pos[u]);
            /* 16x16: the quad's four blocks (sums stay below 2^16: no carry between the halves) */
            lo[u] = FP_DPP(lo[u], 0xB1); hi[u] = FP_DPP(hi[u], 0xB1); /* quad_perm:[1,0,3,2] */
            lo[u] = FP_DPP(lo[u], 0x4E); hi[u] = FP_DPP(hi[u], 0x4E); /* quad_perm:[2,3,0,1] */
            FP_KEYS(b16, lo[u], hi[u], pos[u]);
            /* 32x32: two quads still fit 16 bits; the other half of the row is added half by half into 32-bit sums */
            lo[u] = FP_DPP(lo[u], 0x124); hi[u] = FP_DPP(hi[u], 0x124); /* row_ror:4 */
            const uint32_t lo8 = (uint32_t)__builtin_amdgcn_mov_dpp((int)lo[u], 0x128, 0xf, 0xf, false); /* row_ror:8 */
            const uint32_t hi8 = (uint32_t)__builtin_amdgcn_mov_dpp((int)hi[u], 0x128, 0xf, 0xf, false);
            a0[u] = (lo[u] & 0xffffu) + (lo8 & 0xffffu); a1[u] = (lo[u] >> 16) + (lo8 >> 16);
            a2[u] = (hi[u] & 0xffffu) + (hi8 & 0xffffu); a3[u] = (hi[u] >> 16) + (hi8 >> 16);
            b32 = me_min3(b32, (a0[u] << 12) | pos[u], (a1[u] << 12) | (pos[u] + 1));
            b32 = me_min3(b32, (a2[u] << 12) | (pos[u] + 2), (a3[u] << 12) | (pos[u] + 3));
        }
        SVT_SCHED_FENCE(); /* the 32x32 keys above are done with a0..a3: the sums below run in place */
        /* 64x64: row 1 += row 0, row 3 += row 2 (row_bcast:15), then rows 2, 3 += row 1 (row_bcast:31): complete in lanes 48..63.
         * In place; the first DPP read comes two wait states behind the last write of its operand (s_nop: inline assembly is not
         * covered by the compiler's hazard recogniser), the second round reads what was written four instructions earlier. */
        _Pragma("unroll") for (int u = 0; u < NG; u++)
            __asm__("s_nop 1\n\t"
                    "v_add_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_u32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_u32_dpp %2, %2, %2 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_u32_dpp %3, %3, %3 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
                    "v_add_u32_dpp %1, %1, %1 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
                    "v_add_u32_dpp %2, %2, %2 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
                    "v_add_u32_dpp %3, %3, %3 row_bcast:31 row_mask:0xc bank_mask:0xf"
                    : "+v"(a0[u]), "+v"(a1[u]), "+v"(a2[u]), "+v"(a3[u]));
        _Pragma("unroll") for (int u = 0; u < NG; u++) {
            b64 = me_min3(b64, (a0[u] << 12) | pos[u], (a1[u] << 12) | (pos[u] + 1));
            b64 = me_min3(b64, (a2[u] << 12) | (pos[u] + 2), (a3[u] << 12) | (pos[u] + 3));
        }
    }
#undef FP_KEYS
#undef FP_DPP
    uint64_t *key = c->st->key;
    if (b8 != 0xffffffffu) { /* this wave took at least one group */
        svt_lds_min_u64(&key[21 + z], ((uint64_t)((b8 >> 16) << 1) << 32) | (b8 & 0xffffu));
        if ((z & 3) == 0) svt_lds_min_u64(&key[5 + (z >> 2)], ((uint64_t)((b16 >> 16) << 1) << 32) | (b16 & 0xffffu));
        if ((z & 15) == 0) svt_lds_min_u64(&key[1 + (z >> 4)], ((uint64_t)((b32 >> 12) << 1) << 32) | (b32 & 0xfffu));
        if (z == 63) svt_lds_min_u64(&key[0], ((uint64_t)((b64 >> 12) << 1) << 32) | (b64 & 0xfffu));
    }
}

/* The same phase for the LARGE areas whose width is a multiple of 16 (64 x 64 at the enc-mode <= 5 presets: 1024 groups of four positions
 * per list).  There the layout above is bound by the LDS, not by the vector unit: every group fetches its window again -- twelve 512-byte
 * LDS reads per group and wave, 8.5 cycles each with the two-way bank conflicts of the z-order: 104 K of the phase's 127 K cycles per list
 * (timing builds without the reads / without the QSADs: `profiles/r05_pmc_traffic.md`).  Two changes:
 *   - a lane walks a RUN of four groups (16 positions) along a search row: the six dwords of a window row serve all four (a group's two
 *     operand pairs overlap its neighbours'), three LDS reads instead of eight -- with the source block in registers 3 reads per group
 *     instead of 12;
 *   - a lane is a 16x16 PU (z-order) and one of FOUR runs (lane >> 4) and walks its four 8x8 blocks itself: the 16x16 sums are packed adds inside the lane, the 32x32 sums one packed and one
 *     32-bit quad step, the 64x64 sums two row rotations -- ~19 instructions per group beside its 8 QSADs instead of 48.
 *     (lane >> 4 picks one of four runs that lie UNDER each other, see the loop.)
 * The four runs' minima of a PU sit in four rows of the wave and meet at the end through a swizzle and two-way LDS minima (amortised over
 * the 16 iterations a wave runs per list; the small areas keep the layout above). */
SVT_DEV void me_fullpel_fused16_dev(const me_ctx_t *c, int tid, int sw, int sh) {
    const int rs = c->L.region_stride;
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pg = lane >> 4, b = lane & 15;
    const int bx = ((b & 1) | ((b >> 1) & 2)) * 16, by = (((b >> 1) & 1) | ((b >> 2) & 2)) * 16;
    /* The PUs at by and by + 32 sit in the same LDS banks whatever the row stride (32 rows are a multiple of 32 dwords), and a 32-lane pass
     * holds both: every window read was a two-way bank conflict (half of the phase's LDS-busy cycles, tools/me_phase_lds.sh).  The lower PUs
     * therefore walk their four rows one step ahead (row (r + 1) & 3 where the upper ones take row r: two rows = 70 dwords = 6 banks on, which
     * lands exactly in the banks the other half leaves free) -- a sum does not care about the order of its terms. */
    const int rot = by >> 5;
    uint32_t  sx[4][4], sy[4][4]; /* [8x8 block][step]: the two source dwords of row 2 ((step + rot) & 3) */
    uint32_t  roff[4];            /* byte offset of that row in the window */
    _Pragma("unroll") for (int r = 0; r < 4; r++) roff[r] = (uint32_t)ME_MUL(2 * ((r + rot) & 3), rs);
    _Pragma("unroll") for (int k = 0; k < 4; k++)
        _Pragma("unroll") for (int r = 0; r < 4; r++) {
            const uint2 v = *(const uint2 *)(c->src + ME_MUL(by + (k >> 1) * 8 + 2 * ((r + rot) & 3), ME_SB) + bx + (k & 1) * 8);
            sx[k][r] = v.x; sy[k][r] = v.y;
        }
    const uint32_t rbase = (uint32_t)(c->region - c->lds) + (uint32_t)(ME_MUL(ME_RGN_GY + by, rs) + ME_RGN_GX + bx);
    uint32_t mhi = 0xffff0000u;
    __asm__("" : "+v"(mhi));
    const int      rpr = sw >> 4, nrun = ME_MUL(rpr, sh);           /* runs of 16 positions per search row / in the area */
    const uint32_t inv = me_magics.v[sh];   /* runs are numbered down the columns: the four runs of an iteration lie under each other (see below) */
    uint32_t       b8[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, b16 = 0xffffffffu, b32 = 0xffffffffu, b64 = 0xffffffffu;
#define FQ_DPP(v, ctrl) ((v) + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), 0xf, 0xf, false))
#define FQ_KEYS(bb, lo, hi, pos) do { \
        bb = me_min3(bb, ((lo) << 16) | (pos), ((lo) & mhi) | ((pos) + 1)); \
        bb = me_min3(bb, ((hi) << 16) | ((pos) + 2), ((hi) & mhi) | ((pos) + 3)); } while (0)
    for (int q0 = 4 * w; q0 < nrun; q0 += 16) { /* the waves take four runs at a time, round-robin; a run past the end repeats the last one */
        const int      q = q0 + pg < nrun ? q0 + pg : nrun - 1;
        /* column-major: the lanes of the four runs then differ by whole region rows (39 dwords: every bank offset) instead of by 16 bytes,
         * which on top of the PUs' own 16-byte / 16-row spacing put most of a wave's reads into the same banks (bank-conflict cycles of the
         * phase halved; its time is the vector unit's either way) */
        const int      xr = inv ? (int)__umulhi((uint32_t)q, inv) : q, y = q - ME_MUL(xr, sh);
        const uint32_t pos0 = (uint32_t)(ME_MUL(y, sw) + 16 * xr);
        const uint8_t *rp = c->lds + (rbase + (uint32_t)(ME_MUL(y, rs) + 16 * xr));
        uint32_t       lo[4][4], hi[4][4]; /* [8x8 block][group of the run] */
        _Pragma("unroll") for (int k = 0; k < 4; k++) {
            const uint8_t *wp = rp + ME_MUL((k >> 1) * 8, rs) + (k & 1) * 8;
            uint64_t       acc[4] = {0, 0, 0, 0};
            _Pragma("unroll") for (int r = 0; r < 4; r++) {
                const uint32_t *wr = (const uint32_t *)(wp + roff[r]);
                const uint32_t  d0 = wr[0], d1 = wr[1], d2 = wr[2], d3 = wr[3], d4 = wr[4], d5 = wr[5];
                acc[0] = svt_qsad(((uint64_t)d1 << 32) | d0, sx[k][r], acc[0]); acc[0] = svt_qsad(((uint64_t)d2 << 32) | d1, sy[k][r], acc[0]);
                acc[1] = svt_qsad(((uint64_t)d2 << 32) | d1, sx[k][r], acc[1]); acc[1] = svt_qsad(((uint64_t)d3 << 32) | d2, sy[k][r], acc[1]);
                acc[2] = svt_qsad(((uint64_t)d3 << 32) | d2, sx[k][r], acc[2]); acc[2] = svt_qsad(((uint64_t)d4 << 32) | d3, sy[k][r], acc[2]);
                acc[3] = svt_qsad(((uint64_t)d4 << 32) | d3, sx[k][r], acc[3]); acc[3] = svt_qsad(((uint64_t)d5 << 32) | d4, sy[k][r], acc[3]);
            }
            _Pragma("unroll") for (int j = 0; j < 4; j++) {
                lo[k][j] = (uint32_t)acc[j]; hi[k][j] = (uint32_t)(acc[j] >> 32);
                FQ_KEYS(b8[k], lo[k][j], hi[k][j], pos0 + 4 * j);
            }
        }
        _Pragma("unroll") for (int j = 0; j < 4; j++) {
            const uint32_t pos = pos0 + 4 * j;
            /* 16x16: inside the lane (8 rows x 16 samples x 255 < 2^16: the packed halves do not carry) */
            uint32_t l16 = lo[0][j] + lo[1][j] + lo[2][j] + lo[3][j], h16 = hi[0][j] + hi[1][j] + hi[2][j] + hi[3][j];
            FQ_KEYS(b16, l16, h16, pos);
            /* 32x32: the quad.  Two PUs still fit 16 bits; the second step runs on 32-bit sums */
            l16 = FQ_DPP(l16, 0xB1); h16 = FQ_DPP(h16, 0xB1);                       /* quad_perm:[1,0,3,2] */
            uint32_t a0 = l16 & 0xffffu, a1 = l16 >> 16, a2 = h16 & 0xffffu, a3 = h16 >> 16;
            a0 = FQ_DPP(a0, 0x4E); a1 = FQ_DPP(a1, 0x4E); a2 = FQ_DPP(a2, 0x4E); a3 = FQ_DPP(a3, 0x4E); /* quad_perm:[2,3,0,1] */
            b32 = me_min3(b32, (a0 << 12) | pos, (a1 << 12) | (pos + 1));
            b32 = me_min3(b32, (a2 << 12) | (pos + 2), (a3 << 12) | (pos + 3));
            /* 64x64: the four quads of the run's row of 16 lanes */
            a0 = FQ_DPP(a0, 0x124); a1 = FQ_DPP(a1, 0x124); a2 = FQ_DPP(a2, 0x124); a3 = FQ_DPP(a3, 0x124); /* row_ror:4 */
            a0 = FQ_DPP(a0, 0x128); a1 = FQ_DPP(a1, 0x128); a2 = FQ_DPP(a2, 0x128); a3 = FQ_DPP(a3, 0x128); /* row_ror:8 */
            b64 = me_min3(b64, (a0 << 12) | pos, (a1 << 12) | (pos + 1));
            b64 = me_min3(b64, (a2 << 12) | (pos + 2), (a3 << 12) | (pos + 3));
        }
    }
#undef FQ_KEYS
#undef FQ_DPP
    /* the four runs' minima of a PU: rows pg and pg ^ 1 meet through a swizzle (lane ^ 16), the two halves of the wave in the LDS minimum */
#define FQ_X16(v) do { const uint32_t o_ = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(v), 0x401F); v = o_ < v ? o_ : v; } while (0)
    _Pragma("unroll") for (int k = 0; k < 4; k++) FQ_X16(b8[k]);
    FQ_X16(b16); FQ_X16(b32); FQ_X16(b64);
#undef FQ_X16
    uint64_t *key = c->st->key;
    if ((pg & 1) == 0 && b16 != 0xffffffffu) { /* (a wave that took no run keeps nothing) */
        _Pragma("unroll") for (int k = 0; k < 4; k++) svt_lds_min_u64(&key[21 + 4 * b + k], ((uint64_t)((b8[k] >> 16) << 1) << 32) | (b8[k] & 0xffffu));
        svt_lds_min_u64(&key[5 + b], ((uint64_t)((b16 >> 16) << 1) << 32) | (b16 & 0xffffu));
        if ((b & 3) == 0) svt_lds_min_u64(&key[1 + (b >> 2)], ((uint64_t)((b32 >> 12) << 1) << 32) | (b32 & 0xfffu));
        if (b == 0) svt_lds_min_u64(&key[0], ((uint64_t)((b64 >> 12) << 1) << 32) | (b64 & 0xfffu));
    }
}
#endif

/* two groups per iteration of the fused full-pel loop (independent chains) for the large areas; four were measured on the 64x64 area
 * of C5 and gain nothing (the phase runs at its issue rate there: 44 % of the workgroup's time either way) */
#define ME_FULLPEL_UNROLL2(c) ((c)->p->search_area_width * (c)->p->search_area_height >= 2048)

/* full-pel, search areas whose width is a multiple of 8 (no tail path) with at most 4096 positions: SADs, the nested sums and
 * the per-PU arg-min in ONE phase without the table.  Lane = 8x8 block in z-order, so a DPP quad is a 16x16 PU, a DPP row of
 * 16 lanes a 32x32 PU and the wave the 64x64 PU; the four waves take the groups of 4 positions round-robin.  A lane keeps one
 * running minimum per level as a 32-bit key -- (sad << 16) | position for 8x8 / 16x16 (sums < 2^16), (sad << 12) | position
 * for 32x32 / 64x64 -- and the waves meet in the same 64-bit LDS minimum as ph_fullpel_argmin: unsigned min = the
 * reference's first minimum in raster order. */
SVT_DEV void ph_fullpel_fused(const me_ctx_t *c, int tid, int sw, int sh, int unroll2) {
    (void)unroll2;
    const int rs = c->L.region_stride;
#ifdef SVT_HOST_EMU /* this serial form stands in for me_fullpel_fused_dev / me_fullpel_fused16_dev (the #else); pinned by tests/test_gpu_me.py::test_me_large_search_areas_full_pel_layouts */
    if (tid != 0) return;
    for (int y = 0; y < sh; y++)
        for (int x = 0; x < sw; x++) {
            uint32_t s8[64], s16[16], s32[4] = {0, 0, 0, 0}, s64 = 0;
            for (int z = 0; z < 64; z++) {
                const int bx = ((z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4)) * 8, by = (((z >> 1) & 1) | ((z >> 2) & 2) | ((z >> 3) & 4)) * 8;
                uint32_t  a = 0;
                for (int r = 0; r < 8; r += 2)
                    for (int i = 0; i < 8; i++) {
                        const int d = (int)c->src[(by + r) * ME_SB + bx + i] - (int)c->region[(ME_RGN_GY + y + by + r) * rs + ME_RGN_GX + x + bx + i];
                        a += (uint32_t)(d < 0 ? -d : d);
                    }
                s8[z] = a;
            }
            for (int i = 0; i < 16; i++) s16[i] = (uint16_t)(s8[4 * i] + s8[4 * i + 1] + s8[4 * i + 2] + s8[4 * i + 3]);
            for (int i = 0; i < 16; i++) { s32[i >> 2] += s16[i]; s64 += s16[i]; }
            const uint32_t pos = (uint32_t)(y * sw + x);
            svt_lds_min_u64(&c->st->key[0], ((uint64_t)(2u * s64) << 32) | pos);
            for (int i = 0; i < 4; i++) svt_lds_min_u64(&c->st->key[1 + i], ((uint64_t)(2u * s32[i]) << 32) | pos);
            for (int i = 0; i < 16; i++) svt_lds_min_u64(&c->st->key[5 + i], ((uint64_t)(2u * s16[i]) << 32) | pos);
            for (int i = 0; i < 64; i++) svt_lds_min_u64(&c->st->key[21 + i], ((uint64_t)(2u * s8[i]) << 32) | pos);
        }
#else
    if (unroll2 && (sw & 15) == 0) me_fullpel_fused16_dev(c, tid, sw, sh);
    else if (unroll2) me_fullpel_fused_dev<2>(c, tid, sw, sh);
    else me_fullpel_fused_dev<2, true>(c, tid, sw, sh); /* (the phase's widths are multiples of 8: whole runs) */
#endif
}

/* full-pel: 16x16 sums of every position of the chunk.  In the 8-point path (x < w8) the reference keeps this sum
 * in uint16 (C_DEFAULT/EbComputeSAD_C.c:201,276), in the tail path in 32 bits. */
SVT_DEV void ph_fullpel_sum16(const me_ctx_t *c, int tid, uint32_t *U, int sw, int ny, int w8) {
    (void)c;
    int npos = sw * ny;
    for (int t = tid; t < npos * 16; t += SVT_NT) {
        int             pos = t >> 4, z = t & 15;
        const uint32_t *q   = U + pos * ME_PU_STRIDE + 21 + 2 * z;
        const uint32_t  q0 = q[0], q1 = q[1];
        uint32_t        u   = (q0 & 0xffffu) + (q0 >> 16) + (q1 & 0xffffu) + (q1 >> 16);
        if ((pos % sw) < w8) u = (uint16_t)u;
        U[pos * ME_PU_STRIDE + 5 + z] = u;
    }
}

/* full-pel: 32x32 sums (entries 1..4) and the 64x64 sum (entry 0) per position */
SVT_DEV void ph_fullpel_sum32(const me_ctx_t *c, int tid, uint32_t *U, int npos) {
    (void)c;
    for (int t = tid; t < npos * 5; t += SVT_NT) {
        int             pos = t / 5, j = t - 5 * pos;
        const uint32_t *q   = U + pos * ME_PU_STRIDE + 5;
        uint32_t        u   = 0;
        if (j < 4) u = q[4 * j] + q[4 * j + 1] + q[4 * j + 2] + q[4 * j + 3];
        else _Pragma("unroll") for (int i = 0; i < 16; i++) u += q[i];
        U[pos * ME_PU_STRIDE + (j < 4 ? 1 + j : 0)] = u;
    }
}

/* full-pel: per-PU arg-min.  Thread = (PU, one of 3 interleaved position slices); every PU reads the same table
 * layout, so the scan is branch-free and its loads are independent.  The slices meet in an LDS 64-bit min of
 * (2*sad << 32 | raster index): the unsigned min is exactly the reference's "first minimum in raster order"
 * (strict '<' while scanning positions in raster order). */
SVT_DEV void ph_fullpel_argmin(const me_ctx_t *c, int tid, const uint32_t *U, int sw, int y0, int ny) {
    const int npos = sw * ny;
    const int slice = tid / 85, pu = tid - 85 * slice;
    if (slice < 3) {
        uint32_t bsad = 0xffffffffu, bpos = 0;
        /* dword and bit field of this PU inside a table row */
        const uint32_t *q  = U + (pu < 21 ? pu : 21 + ((pu - 21) >> 1));
        const uint32_t  sh = pu < 21 ? 0u : (uint32_t)((pu - 21) & 1) * 16u, mk = pu < 21 ? 0xffffffffu : 0xffffu;
        for (int pos = slice; pos < npos; pos += 3) {
            uint32_t v = (q[pos * ME_PU_STRIDE] >> sh) & mk;
            if (v < bsad) { bsad = v; bpos = (uint32_t)pos; }
        }
        if (bsad != 0xffffffffu) svt_lds_min_u64(&c->st->key[pu], ((uint64_t)(2u * bsad) << 32) | (uint32_t)(y0 * sw + (int)bpos));
    }
}

#endif
