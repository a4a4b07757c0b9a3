/*
 * me_core.h -- motion estimation of one 64x64 super-block by one 256-thread workgroup (CDNA4 / gfx950).
 *
 * Implements, bit-exactly, the per-SB flow of the reference's motion_estimate_sb
 * (Source/Lib/Codec/EbMotionEstimation.c:4524-5305) for the C_DEFAULT kernels:
 *   test_search_area_bounds (:4260) -> HME level 0/1/2 (:2717-3308, eb_vp9_sad_loop_kernel
 *   C_DEFAULT/EbComputeSAD_C.c:132) -> check_zero_zero_center (:3758) -> full_pel_search_sb (:951,
 *   C_DEFAULT/EbComputeSAD_C.c:193-375, EbMeSadCalculation_C.c:16-99) -> su_pel_enable (:3839) ->
 *   interpolate_search_region_avc (:992, C_DEFAULT/EbAvcStyleMcp_C.c) -> half_pel_search_sb (:1565) ->
 *   quarter_pel_search_sb (:2471) -> bi_prediction_search (:3695) -> candidate ordering (:5186-5293).
 *
 * MI355X mapping
 *   - one workgroup (4 wave64) per SB; both reference lists are processed inside the workgroup because
 *     list 1 starts from list 0's 64x64 motion vector (:4450);
 *   - the 64x64 source SB, the reference search region (+ halo) and its three half-pel planes live in
 *     LDS; every SAD runs out of LDS;
 *   - SADs use v_qsad_pk_u16_u8: one instruction = 4 neighbouring search positions x 4 pixels;
 *     operands are dword-aligned by construction of the LDS layouts (search position 0 sits on a
 *     dword boundary), sub-pel candidates are fetched with v_alignbyte_b32;
 *   - arg-min with the reference's "first minimum in raster order" rule is an order-independent
 *     unsigned min over keys (sad << 32 | raster_index), reduced with ds_min_u64 (LDS atomics);
 *   - integer pixel work, no MFMA.
 *
 * The code is written as a sequence of PHASES.  Inside a phase each of the 256 threads runs a
 * grid-stride loop over independent tasks; phases communicate only through LDS, separated by
 * workgroup barriers.  The uniform control flow between phases reads its inputs from LDS.  This lets
 * the identical source be compiled (a) by hipcc as the device kernel and (b) by a host compiler as a
 * serial emulation used only by the CPU test-suite to debug the kernel logic (tests/emu/).
 *
 * This header keeps the phases every path shares (load, init, centre tests, output) and the driver me_sb_run; the rest is
 *   me_prims.h    the primitives, one body for the GPU (me_prims_dev.h) and one for the emulation (me_prims_emu.h)
 *   me_types.h    me_pic_dev, me_lds_layout, me_state_t, me_ctx_t; mv / PU / search-area geometry
 *   me_tables.h   packed sub-pel candidate tables (+ the emulation's check of them against the reference's)
 *   me_prof.h     ME_MARK and friends in the three profiling builds
 *   me_hme.h      HME level 0/1/2 (:2717-3308)
 *   me_fullpel.h  full_pel_search_sb (:951) and the stand-alone SAD loop
 *   me_subpel.h   interpolation (:992), half / quarter-pel refinement (:1565, :2471), bi-prediction (:3695)
 * Outside me_prims.h a conditional on SVT_HOST_EMU means: a device-only variant of a phase, which the emulation does not run.
 */
#ifndef SVT_ME_CORE_H
#define SVT_ME_CORE_H

#include "me_prims.h"
#include "me_types.h"
#include "me_tables.h"
#include "me_prof.h"
#include "me_hme.h"
#include "me_fullpel.h"
#include "me_subpel.h"

/* ------------------------------------------------------------------------------------------------ */
/* phases (each: grid-stride loop over tasks; tid in [0,256))                                         */
/* ------------------------------------------------------------------------------------------------ */

/* copy a w_bytes x rows rectangle from global memory (any alignment) into LDS (dst 4-byte aligned rows) */
SVT_DEV void ph_load_rect(int tid, uint8_t *dst, int dst_stride, const uint8_t *src, int src_stride, int w_bytes, int rows) {
    /* task = 16 bytes of a row: one global load (four times fewer memory instructions than dwords -- the texture unit's
     * instruction rate, not bandwidth, is what these small rectangles cost), four LDS dword stores; the last unit of a row
     * is shortened to whole dwords so that nothing beyond the rectangle's last dword is read or written.  A thread's
     * (row, unit) pair advances by SVT_NT tasks per step without a division; the loads of two steps are issued before the
     * first LDS store. */
    const int nd = (w_bytes + 3) >> 2, nu = (nd + 3) >> 2, n = nu * rows;
    const int dr = me_udiv(SVT_NT, nu), di = SVT_NT - dr * nu;
    int       r = me_udiv(tid, nu), i = tid - r * nu;
    const me_gsrc g = me_gsrc_of(src);
    for (int t0 = tid; t0 < n; t0 += 2 * SVT_NT) {
        me_u32x4 v[2];
        int      o[2], k[2];
        _Pragma("unroll") for (int u = 0; u < 2; u++) {
            o[u] = -1; k[u] = 0;
            if (t0 + u * SVT_NT < n) {
                const uint32_t goff = (uint32_t)(ME_MUL(r, src_stride) + 16 * i);
                k[u] = nd - 4 * i < 4 ? nd - 4 * i : 4; /* dwords of this unit */
                if (k[u] == 4) v[u] = me_ld128u_g(g.base + goff);
                else {
                    v[u].x = me_gld(g, goff);
                    v[u].y = k[u] > 1 ? me_gld(g, goff + 4) : 0;
                    v[u].z = k[u] > 2 ? me_gld(g, goff + 8) : 0;
                    v[u].w = 0;
                }
                o[u] = r * dst_stride + 16 * i;
            }
            i += di; r += dr;
            if (i >= nu) { i -= nu; r++; }
        }
        _Pragma("unroll") for (int u = 0; u < 2; u++)
            if (o[u] >= 0) {
                uint32_t *d = (uint32_t *)(dst + o[u]);
                d[0] = v[u].x;
                if (k[u] > 1) d[1] = v[u].y;
                if (k[u] > 2) d[2] = v[u].z;
                if (k[u] > 3) d[3] = v[u].w;
            }
    }
}

/* the 1/4-resolution SB, stride 32 */
SVT_DEV void ph_load_quarter(const me_ctx_t *c, int tid) {
    int rows = c->sb_h >> 1, wq = c->sb_w >> 1;
    for (int t = tid; t < rows * 32; t += SVT_NT) {
        int r = t >> 5, x = t & 31;
        c->quarter_sb[t] = x < wq ? *SVT_AS_GLOBAL(const uint8_t, me_pix(&c->pic->cur.quarter, (c->sb_x >> 1) + x, (c->sb_y >> 1) + r)) : 0;
    }
}

/* initial state + decimated SB copies (Codec/EbMotionEstimationProcess.c:984-1035) */
SVT_DEV void ph_init(const me_ctx_t *c, int tid) {
    me_state_t *st = c->st;
    for (int t = tid; t < 85; t += SVT_NT) {
        st->best_mv[0][t] = 0; st->best_mv[1][t] = 0;
        st->best_sad[0][t] = 0; st->best_sad[1][t] = 0;
        st->dir[t] = 0;
    }
    if (tid < 8) st->red[tid] = 0;
    if (tid < 12) { st->hme_x[tid >> 2][tid & 3] = 0; st->hme_y[tid >> 2][tid & 3] = 0; st->hme_sad[tid >> 2][tid & 3] = 0; }
    if (tid == 0) { st->hme_rh = 0; st->hme_xc = 0; st->hme_yc = 0; }
    /* source SB: always 64x64 from the padded picture */
    ph_load_rect(tid, c->src, ME_SB, me_pix(&c->pic->cur.full, c->sb_x, c->sb_y), c->pic->cur.full.stride, ME_SB, ME_SB);
    if (c->p->enable_hme_level_0_flag) {
        /* rows 0,2,4,.. of the 1/16 SB, stride 16 */
        int rows = (c->sb_h >> 2) >> 1, wq = c->sb_w >> 2;
        for (int t = tid; t < rows * 16; t += SVT_NT) {
            int r = t >> 4, x = t & 15;
            st->sixteenth_sb[t] = x < wq ? *SVT_AS_GLOBAL(const uint8_t, me_pix(&c->pic->cur.sixteenth, (c->sb_x >> 2) + x, (c->sb_y >> 2) + 2 * r)) : 0;
        }
    }
    if (c->p->enable_hme_level_1_flag) ph_load_quarter(c, tid);
}

/* Row-subsampled 64-wide SADs of the source SB against up to 5 displaced reference blocks read from
 * global memory (test_search_area_bounds / check_zero_zero_center).  Each thread: one (row, 8-byte) piece.
 * Results accumulate in st->red[k]; caller doubles them. */
SVT_DEV void ph_center_sads(const me_ctx_t *c, int tid, const svt_plane *ref, int ncand, const int16_t *dx, const int16_t *dy) {
    const int rows = c->sb_h >> 1, wq = c->sb_w >> 3; /* 8-byte pieces per row (SB widths are multiples of 8) */
    const int n = rows * wq;                          /* <= 256: one piece per thread */
    uint32_t  acc[5] = {0, 0, 0, 0, 0};
    me_u32x2  v[5], s = {0, 0};
    /* every thread takes part in the wave reductions below; the (independent) global loads of all candidates are issued before
     * the first use: one memory round trip for the phase, one 8-byte load per candidate and thread */
    _Pragma("unroll") for (int k = 0; k < 5; k++) v[k] = s;
    if (tid < n) {
        const int r = me_udiv(tid, wq), i = tid - r * wq;
        const uint32_t *sp = (const uint32_t *)(c->src + (2 * r) * ME_SB + 8 * i);
        s.x = sp[0]; s.y = sp[1];
        const int rstride = ref->stride;
        _Pragma("unroll") for (int k = 0; k < 5; k++) {
            if (k < ncand) {
                const me_gsrc g = me_gsrc_of(me_pix(ref, c->sb_x + dx[k], c->sb_y + dy[k]));
                v[k] = me_ld64u_g(g.base + (uint32_t)(ME_MUL(2 * r, rstride) + 8 * i));
            } else v[k] = s;
        }
    }
    _Pragma("unroll") for (int k = 0; k < 5; k++)
        if (k < ncand) acc[k] = svt_sad4(v[k].y, s.y, svt_sad4(v[k].x, s.x, 0));
    _Pragma("unroll") for (int k = 0; k < 5; k++)
        if (k < ncand) svt_wave_add_u32(&c->st->red[k], acc[k], 1);
}

/* the same row-subsampled SAD for ONE displaced block that already sits in the LDS search region (region byte
 * (col, row) = its top-left sample); result accumulates in st->red[1] */
SVT_DEV void ph_region_center_sad(const me_ctx_t *c, int tid, int col, int row) {
    const int rows = c->sb_h >> 1, wd = c->sb_w >> 2, n = rows * wd, rs = c->L.region_stride;
    uint32_t  acc = 0;
    _Pragma("unroll") for (int h = 0; h < 2; h++) {
        const int t = tid + h * SVT_NT;
        if (t < n) {
            const int r = me_udiv(t, wd), i = t - r * wd;
            acc = svt_sad4(me_ld32u(c->region + ME_MUL(row + 2 * r, rs) + col + 4 * i), *(const uint32_t *)(c->src + (2 * r) * ME_SB + 4 * i), acc);
        }
    }
    svt_wave_add_u32(&c->st->red[1], acc, 1);
}

/* candidate ordering + result record (Codec/EbMotionEstimation.c:5186-5293), one thread per PU */
SVT_DEV void ph_output(const me_ctx_t *c, int tid, svt_me_pu_result *out, uint32_t *out_words) {
    const int sub_sad = c->p->fractional_search_method == SVT_SUB_SAD_SEARCH;
    const int nlist   = c->p->num_ref_lists;
    (void)out;
    for (int pu = tid; pu < 85; pu += SVT_NT) {
        int      n = me_pu_nidx(pu);
        int      total = nlist;
        uint32_t l0 = c->st->best_sad[0][n], l1 = nlist == 2 ? c->st->best_sad[1][n] : 0, bi = 0;
        if (nlist == 2 && me_pu_bipred(c, pu)) {
            bi = c->cand[pu];
            if (sub_sad) bi <<= 1;
            total = 3;
        }
        uint32_t w[10];
        uint32_t mv0 = c->st->best_mv[0][n], mv1 = nlist == 2 ? c->st->best_mv[1][n] : 0;
        w[0] = mv0;
        w[1] = mv1;
        for (int i = 2; i < 10; i++) w[i] = 0;
        if (total == 3) {
            uint32_t v[3] = {l0, l1, bi};
            int      o[3];
            if (l0 <= l1 && l0 <= bi) { o[0] = 0; if (l1 <= bi) { o[1] = 1; o[2] = 2; } else { o[1] = 2; o[2] = 1; } }
            else if (l1 <= l0 && l1 <= bi) { o[0] = 1; if (l0 <= bi) { o[1] = 0; o[2] = 2; } else { o[1] = 2; o[2] = 0; } }
            else if (l0 <= l1) { o[0] = 2; o[1] = 0; o[2] = 1; }
            else { o[0] = 2; o[1] = 1; o[2] = 0; }
            for (int i = 0; i < 3; i++) { w[2 + 2 * i] = v[o[i]]; w[3 + 2 * i] = (uint32_t)o[i]; }
        } else if (total == 2) {
            if (l0 <= l1) { w[2] = l0; w[3] = 0; w[4] = l1; w[5] = 1; }
            else { w[2] = l1; w[3] = 1; w[4] = l0; w[5] = 0; }
        } else {
            w[2] = l0; w[3] = 0;
        }
        w[8] = (uint32_t)total;
        for (int i = 0; i < 10; i++) out_words[pu * 10 + i] = w[i];
    }
}

/* ------------------------------------------------------------------------------------------------ */
/* driver: uniform control flow; PHASE(x) runs x for every thread and ends with a workgroup barrier     */
/* ------------------------------------------------------------------------------------------------ */
SVT_DEV void me_sb_run(const me_ctx_t *c, int tid_) {
    int tid = tid_;
    (void)tid;
    const svt_me_params *p  = c->p;
    me_state_t          *st = c->st;
    const int            nlist = p->num_ref_lists;
    const int            NW = p->number_hme_search_region_in_width, NH = p->number_hme_search_region_in_height;
    ME_PRED0_DECL(); /* list 0 prediction dwords of this lane's bi-pred work, see ph_store_pred0 */
    int16_t  xsc = 0, ysc = 0;
    ME_MARK_BEGIN();

    ME_PHASE(ph_init(c, tid));
    ME_MARK(0);

    for (int list = 0; list < nlist; list++) {
        /* the reference's plane descriptors are read many times (address arithmetic, clipping): keep them in LDS */
        ME_PHASE(if (tid < (int)(3 * sizeof(svt_plane) / 4)) ((uint32_t *)st->refd)[tid] = ((const uint32_t *)&c->pic->ref[list])[tid];
                 if (tid >= 64 && tid < 72) st->red[tid - 64] = 0;
                 /* compact layout: list 0's SSD tables have overwritten the quarter-resolution SB */
                 if (c->L.compact && list == 1 && p->enable_hme_level_1_flag && p->fractional_search_method == SVT_SSD_SEARCH) ph_load_quarter(c, tid));
        const svt_plane  rf_u = me_plane_uni(&st->refd[0]); /* full-resolution reference plane of this list */
        const svt_plane *rf = &rf_u;
        const int        ox = (int16_t)c->sb_x, oy = (int16_t)c->sb_y;
        uint64_t         zero_c = 0; /* 2 * SAD of the block at (0, 0) of this list, when test_search_area_bounds ran */
        int              have_zero = 0;
        if (p->temporal_layer_index > 0 || list == 0) {
            /* ---- test_search_area_bounds ---- */
            {
                const int pad = ME_SB - 1, W = rf->width, H = rf->height;
                const int tw = p->hme_level0_total_search_area_width, th = p->hme_level0_total_search_area_height;
                int16_t   dx[5], dy[5];
                dx[0] = 0; dy[0] = 0;
                dx[1] = me_clip_center(ox, (int16_t)tw, pad, W); dy[1] = me_clip_center(oy, 0, pad, H);
                dx[2] = me_clip_center(ox, 0, pad, W); dy[2] = me_clip_center(oy, (int16_t)(0 - th), pad, H);
                dx[3] = me_clip_center(ox, 0, pad, W); dy[3] = me_clip_center(oy, (int16_t)th, pad, H);
                int16_t dirx = 0, diry = 0;
                int     nc = 4;
                if (list == 1) {
                    const uint32_t mv00 = (uint32_t)ME_UNI(st->best_mv[0][0]);
                    dirx = (int16_t)(0 - (me_mvx(mv00) >> 2));
                    diry = (int16_t)(0 - (me_mvy(mv00) >> 2));
                    dx[4] = me_clip_center(ox, dirx, pad, W); dy[4] = me_clip_center(oy, diry, pad, H);
                    nc = 5;
                }
                ME_PHASE(ph_center_sads(c, tid, rf, nc, dx, dy)); /* red[] was zeroed with the plane descriptors above */
                zero_c = (uint64_t)(uint32_t)ME_UNI(st->red[0]) << 1; have_zero = 1;
                uint64_t b_c = (uint64_t)(uint32_t)ME_UNI(st->red[1]) << 1,
                         c_c = (uint64_t)(uint32_t)ME_UNI(st->red[2]) << 1, d_c = (uint64_t)(uint32_t)ME_UNI(st->red[3]) << 1;
                uint64_t a_c = zero_c; /* [quirk] A is evaluated at the zero-MV address (:4302-4327) */
                uint64_t dir_c = list == 1 ? (uint64_t)(uint32_t)ME_UNI(st->red[4]) << 1 : 0xFFFFFFFFFFFFFull;
                uint64_t best = zero_c;
                if (a_c < best) best = a_c;
                if (b_c < best) best = b_c;
                if (c_c < best) best = c_c;
                if (d_c < best) best = d_c;
                if (dir_c < best) best = dir_c;
                if (best == zero_c) { xsc = 0; ysc = 0; }
                else if (best == a_c) { xsc = (int16_t)(0 - tw); ysc = 0; }
                else if (best == b_c) { xsc = (int16_t)tw; ysc = 0; }
                else if (best == c_c) { xsc = 0; ysc = (int16_t)(0 - th); }
                else if (best == dir_c) { xsc = list ? dirx : 0; ysc = list ? diry : 0; }
                else { xsc = 0; ysc = (int16_t)th; }
                /* red[] is zeroed again when the search region is staged: a barrier must lie between; the HME phases bring theirs */
                if (!(p->enable_hme_flag && c->sb_h == ME_SB && (p->enable_hme_level_0_flag || p->enable_hme_level_1_flag || p->enable_hme_level_2_flag)))
                    ME_PHASE((void)0);
            }
            ME_MARK(1);
            /* ---- HME ---- */
            if (p->enable_hme_flag && c->sb_h == ME_SB) {
                /* The control flow of the hierarchical search (area placement, clipping, batching, scaling, the choice
                 * between the regions) runs on one thread and lives in LDS; the 256 threads only execute the load and
                 * search phases of each batch of windows.  The three levels share one instance of that code. */
                const int last_lvl = p->enable_hme_level_2_flag ? 2 : p->enable_hme_level_1_flag ? 1 : 0;
                int       first = 1, planned = 0;
#define ME_HME_LEVEL_ON(l) ((l) == 0 ? p->enable_hme_level_0_flag : (l) == 1 ? p->enable_hme_level_1_flag : p->enable_hme_level_2_flag)
                for (int lvl = 0; lvl < 3; lvl++) {
                    if (!ME_HME_LEVEL_ON(lvl)) continue;
                    ME_SUBMARK_BEGIN();
                    /* (the plan of every level but the first rides with the previous level's finish: one single-thread section and one
                       barrier less per level) */
#ifndef SVT_HOST_EMU /* device only: me_hme_lanes; the emulation plans on one thread (the line after it); pinned by tests/test_gpu_me.py::test_me_presets_vs_oracle */
                    const int lanes = !(p->single_hme_quadrant && !p->enable_hme_level_1_flag && !p->enable_hme_level_2_flag); /* (the one-region presets keep their short form) */
                    if (!planned && lanes) ME_PHASE(me_hme_lanes(c, tid, list, -1, lvl, xsc, ysc, first));
                    else
#endif
                    if (!planned) ME_UNIFORM_WRITE(me_hme_plan_level(c, list, lvl, xsc, ysc, first));
                    ME_SUBMARK(20);
                    ME_STOP_AT(19);
                    first = 0;
                    me_hme_geom g;
                    me_hme_geom_of(c, list, lvl, &g);
                    const int nbatch = ME_UNI(st->hme_nbatch);
                    for (int b = 0; b < nbatch; b++) {
                        const int         e0 = ME_UNI(st->hme_bstart[b]), e1 = ME_UNI(st->hme_bstart[b + 1]);
                        const me_hme_win *wl = &st->hme_win[e1 - 1];
                        const int         ntl = ME_UNI(wl->tl + ME_HME_UNITS(wl->nd) * wl->rows);
                        const int         nts = ME_UNI(wl->ts + ((g.bw & 3) == 0 ? (wl->sw + 3) >> 2 : wl->sw) * wl->sh);
                        int               slot_mask = 0;
                        for (int e = e0; e < e1; e++) slot_mask |= 1 << st->hme_win[e].slot;
                        slot_mask = ME_UNI(slot_mask);
                        ME_SUBMARK(22);
                        ME_PHASE(ph_hme_load_multi(c, tid, g.ref, st->hme_win, e0, e1, ntl));
                        ME_SUBMARK(14);
                        ME_STOP_AT(20);
                        ME_PHASE(ph_hme_search_multi(c, tid, g.blk, g.bstride, g.bw, g.bh, st->hme_win, e0, e1, nts, st->hme_keys, slot_mask));
                        ME_SUBMARK(15);
                        ME_STOP_AT(21);
                    }
                    ME_SUBMARK(22);
                    int nxt = -1;
                    for (int l2 = lvl + 1; l2 < 3 && nxt < 0; l2++) if (ME_HME_LEVEL_ON(l2)) nxt = l2;
#ifndef SVT_HOST_EMU /* device only: me_hme_lanes; the emulation finishes and plans on one thread (the line after it); pinned by tests/test_gpu_me.py::test_me_presets_vs_oracle */
                    if (lanes) ME_PHASE(me_hme_lanes(c, tid, list, lvl, lvl == last_lvl ? -1 : nxt, xsc, ysc, 0); if (lvl == last_lvl && tid == 0) me_hme_select(c, list));
                    else
#endif
                    ME_UNIFORM_WRITE(me_hme_finish_level(c, lvl); if (lvl == last_lvl) me_hme_select(c, list); else if (nxt >= 0) me_hme_plan_level(c, list, nxt, xsc, ysc, 0));
                    planned = nxt >= 0 && lvl != last_lvl;
                    ME_SUBMARK(21);
                }
#undef ME_HME_LEVEL_ON
                xsc = (int16_t)ME_UNI(st->hme_xc); ysc = (int16_t)ME_UNI(st->hme_yc);
            }
            ME_MARK(2);
        } else {
            xsc = 0; ysc = 0;
        }

        int16_t saw = (int16_t)(p->search_area_width < 127 ? p->search_area_width : 127);
        int16_t sah = (int16_t)(p->search_area_height < 127 ? p->search_area_height : 127);
        int16_t sox, soy;
        int     W, H, w8, tail_extra, loaded = 0;
        /* search area of a centre: position, clipping, derived sizes (Codec/EbMotionEstimation.c:5008-5060) */
#define ME_SET_AREA()                                                                                               \
    do {                                                                                                            \
        saw = (int16_t)(p->search_area_width < 127 ? p->search_area_width : 127);                                    \
        sah = (int16_t)(p->search_area_height < 127 ? p->search_area_height : 127);                                  \
        sox = (int16_t)(xsc - (saw >> 1)); soy = (int16_t)(ysc - (sah >> 1));                                        \
        me_clip_area(ox, &sox, &saw, ME_SB - 1, c->pic_w);                                                           \
        me_clip_area(oy, &soy, &sah, ME_SB - 1, c->pic_h);                                                           \
        W = saw + ME_SB - 1; H = sah + ME_SB - 1; w8 = saw - (saw & 7); tail_extra = (saw & 7) ? 16 : 0;             \
        if (c->L.compact && W + ME_RGN_GX + 4 + tail_extra > c->L.region_stride) { /* no room for the tail columns: the launch with the full layout takes this SB */ \
            if (tid == 0) *SVT_AS_GLOBAL(uint32_t, c->redo) = 1;                                                      \
            return;                                                                                                  \
        }                                                                                                            \
    } while (0)
        /* stage the search region (+ halo) of this list in LDS; the full-pel keys are reset on the way */
#define ME_LOAD_REGION()                                                                                            \
    ME_PHASE(ph_load_rect(tid, c->region, c->L.region_stride, me_pix(rf, c->sb_x + sox - ME_RGN_GX, c->sb_y + soy - ME_RGN_GY), \
                          rf->stride, W + ME_RGN_GX + 4 + tail_extra, H + 2 * ME_RGN_GY + 1);                        \
             for (int t = tid; t < 85; t += SVT_NT) st->key[t] = ((uint64_t)ME_MAX_SAD_VALUE << 32);                  \
             if (tid < 8) st->red[tid] = 0;                                                                          \
             if (tid >= 128 && tid < 137) st->supel[tid - 128] = 0)
        if (xsc != 0 || ysc != 0) {
            /* ---- check_zero_zero_center (:4420-4500): the centre found above against (0, 0).  The SAD at (0, 0) is the
             * one test_search_area_bounds already computed for this list (same function, same block); the SAD at the
             * centre is taken from the search region, which is staged around that centre first -- when the centre
             * wins (the usual case) the region is already in place and no separate global pass is needed ---- */
            xsc = me_clip_center(ox, xsc, ME_SB - 1, rf->width);
            ysc = me_clip_center(oy, ysc, ME_SB - 1, rf->height);
            ME_SET_AREA();
            const int col = ME_RGN_GX + (xsc - sox), row = ME_RGN_GY + (ysc - soy);
            const int inside = have_zero && col >= 0 && row >= 0 && col + c->sb_w <= W + ME_RGN_GX + 4 + tail_extra &&
                               row + c->sb_h <= H + 2 * ME_RGN_GY + 1;
            uint64_t z, h;
            if (inside) {
                ME_LOAD_REGION();
                ME_PHASE(ph_region_center_sad(c, tid, col, row));
                z = zero_c; h = (uint64_t)(uint32_t)ME_UNI(st->red[1]) << 1;
                loaded = 1;
            } else {
                int16_t dx[2], dy[2];
                dx[0] = 0; dy[0] = 0; dx[1] = xsc; dy[1] = ysc;
                ME_PHASE(if (tid < 8) st->red[tid] = 0);
                ME_PHASE(ph_center_sads(c, tid, rf, 2, dx, dy));
                z = (uint64_t)(uint32_t)ME_UNI(st->red[0]) << 1; h = (uint64_t)(uint32_t)ME_UNI(st->red[1]) << 1;
            }
            uint64_t m = z < h ? z : h;
            if (m == z) { xsc = 0; ysc = 0; loaded = 0; }
            if (!loaded) ME_PHASE((void)0); /* everyone has read red[] before the staging below zeroes it */
        }
        ME_MARK(3);
        if (!loaded) {
            ME_SET_AREA();
            ME_LOAD_REGION();
        }
#undef ME_SET_AREA
#undef ME_LOAD_REGION

        ME_MARK(4);
        /* ---- full-pel search, in chunks of search rows ---- */
        {
            uint32_t *U = (uint32_t *)c->planes;
            if (saw >= 8 && (saw & 7) == 0 && saw * sah <= 4096) {
                ME_PHASE(ph_fullpel_fused(c, tid, saw, sah, ME_FULLPEL_UNROLL2(c)));
                ME_MARK(5);
                ME_MARK(6);
            } else {
            int max_pos   = c->L.scratch_bytes / (4 * ME_PU_STRIDE);
            int rows_chunk = max_pos / saw;
            if (rows_chunk < 1) rows_chunk = 1;
            if (rows_chunk > sah) rows_chunk = sah;
            for (int y0 = 0; y0 < sah; y0 += rows_chunk) {
                int ny = y0 + rows_chunk <= sah ? rows_chunk : sah - y0;
                ME_PHASE(ph_fullpel_sad8(c, tid, U, saw, y0, ny, w8));
                ME_PHASE(ph_fullpel_sum16(c, tid, U, saw, ny, w8));
                ME_PHASE(ph_fullpel_sum32(c, tid, U, ny * saw));
                ME_MARK(5);
                ME_PHASE(ph_fullpel_argmin(c, tid, U, saw, y0, ny));
                ME_MARK(6);
            }
            }
            /* keys -> best sad / mv (curr_mv = (y << 18) | (uint16)(x << 2), :108-110) and, where the sub-pel search is gated
             * (su_pel_enable :3839-4258: average MV magnitude / SAD per size class), the nine sums of that decision from the
             * values the lanes have just produced: one PU per lane, wave reductions (st->supel was zeroed with the keys) */
            ME_PHASE(if (tid < 128) {
                const int t = tid;
                uint32_t  mv = 0, sd = 0;
                if (t < 85) {
                    const uint64_t k = st->key[t];
                    const uint32_t idx = (uint32_t)k;
                    if (t == 0 && list == 1) c->cand[0] = 0; /* (after the read: the table may share the keys' bytes) bi-prediction sum of the 64x64 PU */
                    sd = (uint32_t)(k >> 32);
                    st->best_sad[list][t] = sd;
                    if (sd != (uint32_t)ME_MAX_SAD_VALUE) {
                        const int yq = me_udiv((int)idx, saw);
                        int       xi = (int)idx - yq * saw + sox, yi = yq + soy;
                        mv = (((uint32_t)(uint16_t)yi) << 18) | (uint16_t)((uint16_t)xi << 2);
                        st->best_mv[list][t] = mv;
                    } else mv = st->best_mv[list][t];
                }
                if (p->fractional_search_model == 1) {
                    const int cls = t >= 85 ? -1 : t >= 21 ? 2 : t >= 5 ? 1 : t >= 1 ? 0 : -1;
                    _Pragma("unroll") for (int k = 0; k < 3; k++) {
                        svt_wave_add_u32(&st->supel[3 * k + 0], cls == k ? (uint32_t)(int32_t)me_mvx(mv) : 0u, 1);
                        svt_wave_add_u32(&st->supel[3 * k + 1], cls == k ? (uint32_t)(int32_t)me_mvy(mv) : 0u, 1);
                        svt_wave_add_u32(&st->supel[3 * k + 2], cls == k ? sd : 0u, 1);
                    }
                }
            });
        }

        ME_MARK(7);
        /* ---- sub-pel ---- */
        int en32 = 0, en16 = 0, en8 = 0, enq = 0;
        if (p->fractional_search_model == 0) { en32 = en16 = en8 = enq = 1; }
        else if (p->fractional_search_model == 1) {
            int      sx = ME_UNI(st->supel[0]), sy = ME_UNI(st->supel[1]);
            uint32_t ss = (uint32_t)ME_UNI(st->supel[2]);
            uint32_t ax = (uint32_t)(sx >> 2), ay = (uint32_t)(sy >> 2);
            uint32_t mag32 = ax * ax + ay * ay, sad32 = ss >> 2;
            sx = ME_UNI(st->supel[3]); sy = ME_UNI(st->supel[4]); ss = (uint32_t)ME_UNI(st->supel[5]);
            ax = (uint32_t)(sx >> 4); ay = (uint32_t)(sy >> 4);
            uint32_t mag16 = ax * ax + ay * ay, sad16 = ss >> 4;
            sx = ME_UNI(st->supel[6]); sy = ME_UNI(st->supel[7]); ss = (uint32_t)ME_UNI(st->supel[8]);
            ax = (uint32_t)(sx >> 6); ay = (uint32_t)(sy >> 6);
            uint32_t mag8 = ax * ax + ay * ay, sad8 = ss >> 6;
            const int thr_[4]    = {48, 32, 80, 48};
            const int t32_[4][4] = {{1, 0, 1, 0}, {1, 0, 1, 1}, {1, 0, 1, 0}, {1, 1, 1, 0}};
            const int t16_[4]    = {0, 1, 0, 1};
            const int t8_[4][4]  = {{0, 1, 0, 1}, {0, 1, 0, 1}, {0, 1, 0, 1}, {0, 1, 0, 0}};
            int       tl = p->temporal_layer_index > 3 ? 3 : p->temporal_layer_index;
            uint32_t  t2 = (uint32_t)(thr_[tl] * thr_[tl]);
            en32 = t32_[tl][2 * !(mag32 < t2) + !(sad32 < 32 * 32 * 6)];
            en16 = t16_[2 * !(mag16 < t2) + !(sad16 < 16 * 16 * 2)];
            en8  = t8_[tl][2 * !(mag8 < t2) + !(sad8 < 8 * 8 * 2)];
            enq  = 1;
        }
        const int need_planes = en32 || en16 || en8 || enq || (nlist == 2);
        ME_MARK(8);
        if (need_planes) {
            ME_PHASE(ph_interp_strips(c, tid, W, H));
        }
        ME_MARK(9);
#ifndef SVT_HOST_EMU /* device only: ph_subpel_fast and fast_bi; the emulation takes the task lists below and ph_store_pred0 / ph_bipred; pinned by tests/test_gpu_me.py::test_me_presets_vs_oracle */
        /* SUB_SAD refinement of the 32x32 / 16x16 PUs only (the M5+ presets): one phase, see ph_subpel_fast */
        /* with cu8x8_mode == 1 that holds for both lists whatever the gating says: the 32x32 / 16x16 levels of the bi-prediction
         * ride on the same lanes (fast_bi), the 64x64 level stays with ph_store_pred0 / ph_bipred */
        const int fast_bi = nlist == 2 && p->fractional_search_model != 2 && p->fractional_search_method == SVT_SUB_SAD_SEARCH &&
                            !p->fractional_search64x64 && p->cu16x16_mode == 0 && p->cu8x8_mode == 1;
        if (enq && p->fractional_search_method == SVT_SUB_SAD_SEARCH && !p->fractional_search64x64 && p->cu16x16_mode == 0 &&
            !(en8 && p->cu8x8_mode != 1)) {
            if (en32 || en16 || fast_bi) ME_PHASE(ph_subpel_fast(c, tid, list, sox, soy, en32, en16, fast_bi, ME_PRED0_REGS));
            ME_MARK(10);
            ME_MARK(11);
        } else
#else
        const int fast_bi = 0;
#endif
        if (en32 || en16 || en8 || enq) {
            ME_PHASE(me_cand_zero(c, tid, 0);
                     ph_subpel_prep(c, tid, en32, en16, en8));
            ME_PHASE(ph_halfpel(c, tid, list, sox, soy, en32, en16, en8));
            ME_PHASE(ph_halfpel_decide(c, tid, list, en32, en16, en8));
            ME_MARK(10);
            if (enq) {
                ME_PHASE(me_cand_zero(c, tid, 1));
                ME_PHASE(ph_quarterpel(c, tid, list, sox, soy, en32, en16, en8));
                ME_PHASE(ph_quarterpel_decide(c, tid, list, en32, en16, en8));
            }
            ME_MARK(11);
        }
        if (nlist == 2) {
            const int lmax = fast_bi ? 0 : 4, czero = 85; /* fast_bi: every level is done, cand[0..20] hold the sums */
            if (lmax == 0) { /* nothing left */ }
            else if (list == 0) ME_PHASE(ph_store_pred0(c, tid, sox, soy, ME_PRED0_REGS, lmax));
            else {
                ME_PHASE(for (int t = tid; t < czero; t += SVT_NT) c->cand[t] = 0);
                ME_PHASE(ph_bipred(c, tid, sox, soy, ME_PRED0_REGS, lmax));
            }
            ME_MARK(12);
        }
    }

    /* ---- results ---- */
    uint32_t *ow = (uint32_t *)c->planes;
    ME_PHASE(ph_output(c, tid, 0, ow));
    {
        uint32_t SVT_GLOBAL *g = SVT_AS_GLOBAL(uint32_t, c->pic->results + (size_t)c->sb_index * 85);
        ME_TASKS(t, 850) g[t] = ow[t];
        if (c->pic->rcme && tid == 0) {
            uint32_t acc = 0;
            for (int i = 0; i < 16; i++) acc += ow[(5 + i) * 10 + 2];
            *SVT_AS_GLOBAL(uint32_t, &c->pic->rcme[c->sb_index]) = acc;
        }
    }
    ME_MARK(13);
}

#endif /* SVT_ME_CORE_H */
