/* me_subpel.h -- everything behind the integer search of a list: the half-pel planes (interpolate_search_region_avc), the half- and
 * quarter-pel refinement (candidate tasks + decisions, or the one-phase device form), the list predictions and bi_prediction_search. */
#ifndef SVT_ME_SUBPEL_H
#define SVT_ME_SUBPEL_H
#include "me_tables.h"

SVT_DEV uint8_t me_clip8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
SVT_DEV uint8_t me_tap4(int a, int b, int d, int e) { return me_clip8((-2 * a + 18 * b + 18 * d - 2 * e + 16) >> 5); }

/* Half-pel planes (interpolate_search_region_avc, Codec/EbMotionEstimation.c:992-1070; C_DEFAULT/EbAvcStyleMcp_C.c:25-73), natural
 * coordinates with a guard of ME_PL_G samples: B (x + 1/2, y) = 4-tap filter along the region row, H (x, y + 1/2) = the same filter
 * down the region's columns, J (x + 1/2, y + 1/2) = the vertical filter over B, defined for y in [-1, H - 1].  Plane column px is
 * region column px + 2 (ME_RGN_GX - ME_PL_G), so the 7 region bytes a B dword needs sit in two aligned region dwords. */
/* ---- the three half-pel planes in ONE pass over column strips ----
 * A thread owns one dword column of the planes and a run of rows, and walks DOWN the region: region row R (two aligned dwords)
 * yields, in 16-bit lanes, the horizontal half-pel samples B(R - 1) and the samples the vertical filter needs from that row;
 * a window of the last four rows then gives H(R - 3) (vertical filter of the region) and J(R - 3) (vertical filter of B)
 * without re-reading anything: 2 LDS reads and 3 writes per output dword triple (a phase per plane pair needed 12 and 3, and
 * permuted every operand again for H and J). */
SVT_DEV void ph_interp_strips(const me_ctx_t *c, int tid, int W, int H) {
    const int rs = c->L.region_stride, ps = c->L.plane_stride, pb = c->L.plane_bytes, pwd = (W + 2 * ME_PL_G + 3) >> 2, ph = H + 2 * ME_PL_G;
    const int nseg = me_udiv(SVT_NT, pwd), per = me_udiv(ph + nseg - 1, nseg);
    const int seg = me_udiv(tid, pwd), j = tid - seg * pwd;
    const int r0 = ME_MUL(seg, per), cnt = r0 + per < ph ? per : ph - r0; /* this strip: plane rows r0 .. r0 + cnt - 1 */
    if (seg >= nseg || cnt <= 0) return;
    /* Plane row py (natural row py - ME_PL_G) takes: B(py) from region row py + 1 (horizontal filter along it); H(py) and J(py)
     * from region rows py .. py + 3 -- H filters the rows themselves vertically, J the B rows derived from them (B(py - 1) ..
     * B(py + 2)).  Step i of the walk reads region row r0 + i (i = 0 .. cnt + 2), stores B(r0 + i - 1) and completes the window
     * of H / J(r0 + i - 3).  The window is a ring of four slots indexed by i & 3; the walk is unrolled by four so that every slot
     * is a named register (no moves) and the row offsets are immediates where the strides are. */
    uint32_t ve[4], vo[4], be[4], bo[4]; /* per window row: its samples for the vertical filter (even / odd), and the B row it yields */
    _Pragma("unroll") for (int k = 0; k < 4; k++) { ve[k] = vo[k] = be[k] = bo[k] = 0; }
    const uint8_t *rp = c->region + 4 * j + ME_MUL(r0, rs);      /* region row r0 + i0 */
    uint8_t       *wp = c->planes + 4 * j + ME_MUL(r0 - 3, ps);  /* plane row r0 + i0 - 3 of B (H, J: + pb, + 2 pb) */
    const int      jlo = 4 - r0, jhi = H + 5 - r0;               /* J exists for plane rows 1 .. H + 1: i in [jlo, jhi) */
    for (int i0 = 0; i0 < per + 3; i0 += 4) {                    /* same trip count in every lane; the stores carry the lane's bounds */
        _Pragma("unroll") for (int u = 0; u < 4; u++) {
            const int       i = i0 + u;
            if (i >= per + 3) break; /* (uniform: the walk is per + 3 steps long; unrolled by four it used to run up to three steps past its end) */
            const uint32_t *rw = (const uint32_t *)(rp + u * rs);
            const uint32_t  lo = rw[0], hi = rw[1];
            /* P(k) = bytes (k, k + 2) of the row's 8 bytes in 16-bit lanes: horizontal taps of the even outputs are P1..P4, of the
             * odd ones P2..P5; the vertical filter works on bytes 2..5 = P2 (even) and P3 (odd) */
            const uint32_t  p1 = me_pair16(hi, lo, 1), p2 = me_pair16(hi, lo, 2), p3 = me_pair16(hi, lo, 3), p4 = me_pair16(hi, lo, 4), p5 = me_pair16(hi, lo, 5);
            const uint32_t  he = me_tap4_half(p1, p2, p3, p4), ho = me_tap4_half(p2, p3, p4, p5);
            if (i >= 1 && i <= cnt) *(uint32_t *)(wp + (u + 2) * ps) = me_half_join(he, ho);
            ve[u] = p2; vo[u] = p3; be[u] = me_half_lanes(he); bo[u] = me_half_lanes(ho);
            if (i >= 3 && i < cnt + 3) {
                const int o = (u + 1) & 3, a = (u + 2) & 3, b = (u + 3) & 3; /* oldest .. newest = o, a, b, u */
                *(uint32_t *)(wp + u * ps + pb) = me_half_join(me_tap4_half(ve[o], ve[a], ve[b], ve[u]), me_tap4_half(vo[o], vo[a], vo[b], vo[u]));
                if (i >= jlo && i < jhi)
                    *(uint32_t *)(wp + u * ps + 2 * pb) = me_half_join(me_tap4_half(be[o], be[a], be[b], be[u]), me_tap4_half(bo[o], bo[a], bo[b], bo[u]));
            }
        }
        rp += 4 * rs; wp += 4 * ps;
    }
}

/* byte pointer (LDS) of plane `id` at natural position (x, y) relative to the region's top-left */
SVT_DEV int me_plane_stride(const me_ctx_t *c, int id) { return id == ME_PF ? c->L.region_stride : c->L.plane_stride; }
SVT_DEV const uint8_t *me_plane_at(const me_ctx_t *c, int id, int x, int y) {
    if (id == ME_PF) return c->region + ME_MUL(ME_RGN_GY + y, c->L.region_stride) + ME_RGN_GX + x;
    return c->planes + ME_MUL(id - 1, c->L.plane_bytes) + ME_MUL(y + ME_PL_G, c->L.plane_stride) + x + ME_PL_G;
}

/* SAD of a w x rows block: src rows at stride ss (LDS, dword aligned) vs candidate at any byte alignment (stride csa,
 * a multiple of 4), optionally averaged with a second candidate plane (b != 0, stride csb).  Each candidate row is fetched as
 * w/4 + 1 aligned dwords and shifted into place with v_alignbyte.  ssd_out != 0: also the sum of squared differences
 * (eb_vp9_spatial_full_distortion_kernel, C_DEFAULT/EbPictureOperators_C.c:337-356; averaging form
 * Codec/EbMotionEstimation.c:1708-1725). */
SVT_DEV uint32_t me_block_sad_rows(const uint8_t *src, int ss, const uint8_t *a, const uint8_t *b, int csa, int csb, int w, int r0, int r1, uint32_t *ssd_out) {
    uint32_t        sad = 0, ssd = 0;
    const uint32_t  sha = (uint32_t)((uintptr_t)a & 3), shb = b ? (uint32_t)((uintptr_t)b & 3) : 0;
    const uint8_t  *a0 = a - sha, *b0 = b ? b - shb : a0;
    const int       n = w >> 2;
    for (int r = r0; r < r1; r++) {
        const uint32_t *s  = (const uint32_t *)(src + ME_MUL(r, ss));
        const uint32_t *pa = (const uint32_t *)(a0 + ME_MUL(r, csa)), *pb = (const uint32_t *)(b0 + ME_MUL(r, csb));
        uint32_t        la = pa[0], lb = b ? pb[0] : 0;
        for (int i = 0; i < n; i++) {
            uint32_t ha = pa[i + 1];
            uint32_t va = svt_alignbyte(ha, la, sha);
            la = ha;
            if (b) {
                uint32_t hb = pb[i + 1];
                uint32_t vb = svt_alignbyte(hb, lb, shb);
                lb = hb;
                va = svt_avg4(va, vb); /* per-byte (a + b + 1) >> 1 */
            }
            sad = svt_sad4(va, s[i], sad);
            if (ssd_out) ssd = svt_ssd4(va, s[i], ssd);
        }
    }
    if (ssd_out) *ssd_out = ssd;
    return sad;
}

/* direction codes, Codec/EbMotionEstimation.c:34-41 */
enum { ME_D_TL = 0, ME_D_T = 1, ME_D_TR = 2, ME_D_R = 3, ME_D_BR = 4, ME_D_B = 5, ME_D_BL = 6, ME_D_L = 7 };

/* which PUs are refined for the current list (half_pel_search_sb :1565-1702 gating) */
SVT_DEV int me_pu_refined(const me_ctx_t *c, int pu, int en32, int en16, int en8) {
    if (pu == 0) return c->p->fractional_search64x64;
    if (pu < 5) return en32;
    if (pu < 21) return en16 && c->p->cu16x16_mode == 0;
    return en8 && c->p->cu8x8_mode != 1;
}

/* lanes cooperating on one candidate block (row-interleaved) */
#define ME_SUB_LANES 8

/* the refined PUs of the current list as a dense index space: k in [0, me_active_count) -> raster pu */
SVT_DEV int me_active_count(const me_ctx_t *c, int en32, int en16, int en8, int *n64, int *n32, int *n16) {
    *n64 = c->p->fractional_search64x64 ? 1 : 0;
    *n32 = en32 ? 4 : 0;
    *n16 = (en16 && c->p->cu16x16_mode == 0) ? 16 : 0;
    return *n64 + *n32 + *n16 + ((en8 && c->p->cu8x8_mode != 1) ? 64 : 0);
}
SVT_DEV int me_active_pu(int k, int n64, int n32, int n16) {
    if (k < n64) return 0;
    k -= n64;
    if (k < n32) return 1 + k;
    k -= n32;
    if (k < n16) return 5 + k;
    return 21 + k - n16;
}

/* one record per refined PU so that the candidate tasks start from two LDS reads instead of re-deriving the PU from
 * its dense index (range tests, z-order interleave) under divergent branches */
SVT_DEV void ph_subpel_prep(const me_ctx_t *c, int tid, int en32, int en16, int en8) {
    int       n64, n32, n16;
    const int nact = me_active_count(c, en32, en16, en8, &n64, &n32, &n16);
    for (int k = tid; k < nact; k += SVT_NT) {
        const int pu = me_active_pu(k, n64, n32, n16);
        int       px, py, w;
        me_pu_geom(pu, &px, &py, &w);
        c->st->spu[k] = (uint32_t)pu | ((uint32_t)me_pu_nidx(pu) << 7) | ((uint32_t)(px >> 3) << 14) | ((uint32_t)(py >> 3) << 17) |
                        ((uint32_t)(w == 8 ? 0 : w == 16 ? 1 : w == 32 ? 2 : 3) << 20);
    }
}
#define ME_SPU_PU(i) ((int)((i) & 127))
#define ME_SPU_N(i) ((int)(((i) >> 7) & 127))
#define ME_SPU_PX(i) ((int)(((i) >> 14) & 7) << 3)
#define ME_SPU_PY(i) ((int)(((i) >> 17) & 7) << 3)
#define ME_SPU_W(i) (8 << (((i) >> 20) & 3))

/* Sub-pel work split: a candidate block of a 64x64 PU is shared by 16 lanes, of a 32x32 PU by 4 lanes, a 16x16 or 8x8
 * candidate is one lane's job (8 or 4 rows of 16 or 8 samples) -- at the BASELINE settings that is exactly 256 tasks of
 * equal size per half-pel pass.  The dense PU index k runs 64x64, 32x32, 16x16, 8x8 (me_active_pu), so the task ranges of
 * the three lane counts are contiguous.  t -> (k, candidate index, sub-lane, lanes per candidate); returns 0 past the end. */
/* lanes per candidate block: 16 for 64x64, 4 for 32x32, 1 below.  With the 21 PUs and 8 candidates of the M8 / M9 presets
 * that is 384 tasks = one and a half passes of the workgroup; 8 / 2 / 1 (exactly one pass of tasks twice as long) was
 * measured slower (ME 2.30 instead of 2.24 ms per mini-GOP): the longer serial row loops expose more LDS latency than the
 * half-empty second pass costs */
#define ME_HP_NL64 16
#define ME_HP_NL32 4
SVT_DEV int me_subpel_task(int t, int ncand, int n64, int n32, int nrest, int *k, int *ci, int *sl, int *nl) {
    const int T64 = n64 * ncand * ME_HP_NL64, T32 = n32 * ncand * ME_HP_NL32;
    int       q, base;
    if (t < T64) { *nl = ME_HP_NL64; *sl = t & (ME_HP_NL64 - 1); q = t / ME_HP_NL64; base = 0; }
    else if (t < T64 + T32) { const int u = t - T64; *nl = ME_HP_NL32; *sl = u & (ME_HP_NL32 - 1); q = u / ME_HP_NL32; base = n64; }
    else { q = t - T64 - T32; *nl = 1; *sl = 0; base = n64 + n32; if (q >= nrest * ncand) return 0; }
    const int kk = ncand == 8 ? q >> 3 : ncand == 3 ? q / 3 : q / 9;
    *k = base + kk; *ci = q - kk * ncand;
    return 1;
}

/* The sub-pel candidate table: entry k = pu * 8 + candidate.  Entries of the PUs 0..20 are dwords; those of the 8x8 PUs (k >= 168,
 * refined only when cu8x8_mode != 1) are halfwords -- an 8x8 SAD is at most 64 x 255 -- two to a dword at c->cand_hi: 1 KB instead of 2. */
SVT_DEV uint32_t me_cand_get(const me_ctx_t *c, int k) {
    if (k < 168) return c->cand[k];
    k -= 168;
    return (c->cand_hi[k >> 1] >> (16 * (k & 1))) & 0xffffu;
}
SVT_DEV uint32_t *me_cand_slot(const me_ctx_t *c, int k, int *shift) {
    if (k < 168) { *shift = 0; return &c->cand[k]; }
    k -= 168;
    *shift = 16 * (k & 1);
    return &c->cand_hi[k >> 1];
}
/* zero the table (and the candidate SSDs: keep_best = 1 leaves entry 8 of every PU, its best SSD so far) */
SVT_DEV void me_cand_zero(const me_ctx_t *c, int tid, int keep_best) {
    for (int t = tid; t < 85 * 9; t += SVT_NT) {
        if (t < (c->L.cand_dwords < 168 ? c->L.cand_dwords : 168)) c->cand[t] = 0;
        if (c->L.off_cand_hi >= 0 && t < 256) c->cand_hi[t] = 0;
        if (c->ssdc && !(keep_best && me_udiv(t, 9) * 9 + 8 == t)) c->ssdc[t] = 0;
    }
}

/* half-pel: distortion of every candidate accumulates in st->cand[pu*8+cand] (pre-zeroed).
 * SUB_SAD: rows 0,2,4.. only, doubled by the consumer; FULL_SAD: all rows.  SSD_SEARCH: 9 candidates per PU (8 = the
 * integer position, whose SSD seeds the comparison, :1107-1160), all rows, SAD in st->cand and SSD in c->ssdc. */
SVT_DEV void ph_halfpel(const me_ctx_t *c, int tid, int list, int sox, int soy, int en32, int en16, int en8) {
    const int sub_sad = c->p->fractional_search_method == SVT_SUB_SAD_SEARCH;
    const int ssd     = c->p->fractional_search_method == SVT_SSD_SEARCH;
    const int ncand   = ssd ? 9 : 8;
    int       n64, n32, n16;
    const int nact = me_active_count(c, en32, en16, en8, &n64, &n32, &n16);
    const int total = ncand * (n64 * ME_HP_NL64 + n32 * ME_HP_NL32 + (nact - n64 - n32));
    for (int t = tid; t < total; t += SVT_NT) {
        int k, cand, sl, nl;
        if (!me_subpel_task(t, ncand, n64, n32, nact - n64 - n32, &k, &cand, &sl, &nl)) break;
        const uint32_t info = c->st->spu[k];
        const int      pu = ME_SPU_PU(info), n = ME_SPU_N(info), px = ME_SPU_PX(info), py = ME_SPU_PY(info), w = ME_SPU_W(info);
        uint32_t mv = c->st->best_mv[list][n];
        int      xs = (int16_t)((me_mvx(mv) >> 2) - (int16_t)sox) + px;
        int      ys = (int16_t)((me_mvy(mv) >> 2) - (int16_t)soy) + py;
        int            hpl = ME_PF, hdx = 0, hdy = 0;
        if (cand < 8) me_hcand_get(cand, &hpl, &hdx, &hdy);
        const uint8_t *cp = me_plane_at(c, hpl, xs + hdx, ys + hdy);
        const uint8_t *sp = c->src + py * ME_SB + px;
        const int      rows = sub_sad ? (w >> 1) : w, step = sub_sad ? 2 : 1;
        const int      per = nl == ME_HP_NL64 ? rows / ME_HP_NL64 : nl == ME_HP_NL32 ? rows / ME_HP_NL32 : rows, r0 = sl * per;
        uint32_t e = 0;
        const int cs = me_plane_stride(c, hpl) * step;
        uint32_t d = me_block_sad_rows(sp, ME_SB * step, cp, 0, cs, cs, w, r0, r0 + per, ssd ? &e : 0);
        if (cand < 8) { int sh; uint32_t *slot = me_cand_slot(c, pu * 8 + cand, &sh); svt_group_add_var(slot, d << sh, nl); }
        if (ssd) svt_group_add_var(&c->ssdc[pu * 9 + cand], e, nl);
    }
}

/* half-pel decision per PU: sequential strict '<' updates in test order, then direction with the tie
 * order L,R,T,B,TL,TR,BL,BR (:1531-1556).  SSD_SEARCH compares SSDs and records the winner's SAD. */
SVT_DEV void ph_halfpel_decide(const me_ctx_t *c, int tid, int list, int en32, int en16, int en8) {
    const int sub_sad = c->p->fractional_search_method == SVT_SUB_SAD_SEARCH;
    const int ssd     = c->p->fractional_search_method == SVT_SSD_SEARCH;
    for (int pu = tid; pu < 85; pu += SVT_NT) {
        if (!me_pu_refined(c, pu, en32, en16, en8)) continue;
        int      n    = me_pu_nidx(pu);
        uint32_t best = c->st->best_sad[list][n], mv = c->st->best_mv[list][n];
        uint32_t bssd = ssd ? c->ssdc[pu * 9 + 8] : 0;
        int16_t  xm = me_mvx(mv), ym = me_mvy(mv);
        uint32_t d[8];
        for (int i = 0; i < 8; i++) {
            int sx, sy;
            me_dmv_get(i, &sx, &sy);
            if (ssd) {
                d[i] = c->ssdc[pu * 9 + i];
                if (d[i] < bssd) { bssd = d[i]; best = me_cand_get(c, pu * 8 + i); mv = me_pack_mv(xm + 2 * sx, ym + 2 * sy); }
            } else {
                d[i] = me_cand_get(c, pu * 8 + i);
                if (sub_sad) d[i] <<= 1;
                if (d[i] < best) { best = d[i]; mv = me_pack_mv(xm + 2 * sx, ym + 2 * sy); }
            }
        }
        uint32_t m = d[0];
        for (int i = 1; i < 8; i++) if (d[i] < m) m = d[i];
        uint8_t dir;
        if (m == d[0]) dir = ME_D_L;
        else if (m == d[1]) dir = ME_D_R;
        else if (m == d[2]) dir = ME_D_T;
        else if (m == d[3]) dir = ME_D_B;
        else if (m == d[4]) dir = ME_D_TL;
        else if (m == d[5]) dir = ME_D_TR;
        else if (m == d[7]) dir = ME_D_BL;
        else dir = ME_D_BR;
        c->st->best_sad[list][n] = best;
        c->st->best_mv[list][n]  = mv;
        c->st->dir[n]            = dir;
        if (ssd) c->ssdc[pu * 9 + 8] = bssd; /* (the thread that read the integer position's SSD there) */
    }
}

SVT_DEV int me_qvalid(int in_half, int dir, int pos) {
    /* pos: 0 L,1 R,2 T,3 B,4 TL,5 TR,6 BR,7 BL (:1761-1796) */
    int v_tl, v_t, v_tr, v_r, v_br, v_b, v_bl, v_l;
    if (in_half) {
        v_tl = dir == ME_D_R || dir == ME_D_BR || dir == ME_D_B;
        v_t  = dir == ME_D_BR || dir == ME_D_B || dir == ME_D_BL;
        v_tr = dir == ME_D_B || dir == ME_D_BL || dir == ME_D_L;
        v_r  = dir == ME_D_BL || dir == ME_D_L || dir == ME_D_TL;
        v_br = dir == ME_D_L || dir == ME_D_TL || dir == ME_D_T;
        v_b  = dir == ME_D_TL || dir == ME_D_T || dir == ME_D_TR;
        v_bl = dir == ME_D_T || dir == ME_D_TR || dir == ME_D_R;
        v_l  = dir == ME_D_TR || dir == ME_D_R || dir == ME_D_BR;
    } else {
        v_tl = dir == ME_D_L || dir == ME_D_TL || dir == ME_D_T;
        v_t  = dir == ME_D_TL || dir == ME_D_T || dir == ME_D_TR;
        v_tr = dir == ME_D_T || dir == ME_D_TR || dir == ME_D_R;
        v_r  = dir == ME_D_TR || dir == ME_D_R || dir == ME_D_BR;
        v_br = dir == ME_D_R || dir == ME_D_BR || dir == ME_D_B;
        v_b  = dir == ME_D_BR || dir == ME_D_B || dir == ME_D_BL;
        v_bl = dir == ME_D_B || dir == ME_D_BL || dir == ME_D_L;
        v_l  = dir == ME_D_BL || dir == ME_D_L || dir == ME_D_TL;
    }
    switch (pos) {
    case 0: return v_l; case 1: return v_r; case 2: return v_t; case 3: return v_b;
    case 4: return v_tl; case 5: return v_tr; case 6: return v_br; default: return v_bl;
    }
}

/* quarter-pel: task = (refined pu, j 0..2, sub-lane): the three positions around the half-pel direction.
 * The direction codes TL,T,TR,R,BR,B,BL,L run clockwise, and me_qvalid() accepts position X when
 * X is within one step of dir (integer best) or of the opposite of dir (half-pel best) (:1761-1796).
 * [quirk] the 64x64 PU is evaluated on its top-left 32x32 (:2525-2526). */
SVT_DEV void ph_quarterpel(const me_ctx_t *c, int tid, int list, int sox, int soy, int en32, int en16, int en8) {
    const int sub_sad = c->p->fractional_search_method == SVT_SUB_SAD_SEARCH;
    const int ssd     = c->p->fractional_search_method == SVT_SSD_SEARCH;
    int       n64, n32, n16;
    const int nact = me_active_count(c, en32, en16, en8, &n64, &n32, &n16);
    /* few candidates (3 per PU): 8 lanes share one candidate block so that the pass stays short */
    for (int t = tid; t < nact * 3 * ME_SUB_LANES; t += SVT_NT) {
        const int sl = t % ME_SUB_LANES, q = t / ME_SUB_LANES, k = q / 3, j = q - 3 * k, nl = ME_SUB_LANES;
        const uint32_t info = c->st->spu[k];
        const int      pu = ME_SPU_PU(info), n = ME_SPU_N(info), px = ME_SPU_PX(info), py = ME_SPU_PY(info);
        const int      w = pu == 0 ? 32 : ME_SPU_W(info);
        uint32_t mv = c->st->best_mv[list][n];
        int16_t  xm = me_mvx(mv), ym = me_mvy(mv);
        int      method = (ym & 2) + ((xm & 2) >> 1);
        int      dirx = ((method != 0 ? c->st->dir[n] ^ 4 : c->st->dir[n]) + j - 1) & 7;
        int      pos  = (int)(0x07361524u >> (4 * dirx)) & 7; /* direction code -> L,R,T,B,TL,TR,BR,BL index */
        int xs = (int16_t)(((xm + 2) >> 2) - (int16_t)sox) + px;
        int ys = (int16_t)(((ym + 2) >> 2) - (int16_t)soy) + py;
        const uint32_t e  = me_qtab_get(method, pos);
        const uint8_t *a  = me_plane_at(c, (int)(e & 3), xs - (int)((e >> 2) & 1), ys - (int)((e >> 3) & 1));
        const uint8_t *b  = me_plane_at(c, (int)((e >> 4) & 3), xs - (int)((e >> 6) & 1), ys - (int)((e >> 7) & 1));
        const uint8_t *sp = c->src + py * ME_SB + px;
        const int      rows = sub_sad ? (w >> 1) : w, step = sub_sad ? 2 : 1;
        const int      per = (rows + nl - 1) / nl, r0 = sl * per, r1 = r0 + per < rows ? r0 + per : rows;
        uint32_t sq = 0;
        uint32_t d = r0 < r1 ? me_block_sad_rows(sp, ME_SB * step, a, b, me_plane_stride(c, (int)(e & 3)) * step,
                                                 me_plane_stride(c, (int)((e >> 4) & 3)) * step, w, r0, r1, ssd ? &sq : 0) : 0;
        { int sh; uint32_t *slot = me_cand_slot(c, pu * 8 + pos, &sh); svt_group_add_u32(slot, d << sh, nl); }
        if (ssd) svt_group_add_u32(&c->ssdc[pu * 9 + pos], sq, nl);
    }
}

SVT_DEV void ph_quarterpel_decide(const me_ctx_t *c, int tid, int list, int en32, int en16, int en8) {
    const int sub_sad = c->p->fractional_search_method == SVT_SUB_SAD_SEARCH;
    const int ssd     = c->p->fractional_search_method == SVT_SSD_SEARCH;
    for (int pu = tid; pu < 85; pu += SVT_NT) {
        if (!me_pu_refined(c, pu, en32, en16, en8)) continue;
        int      n    = me_pu_nidx(pu);
        uint32_t best = c->st->best_sad[list][n], mv = c->st->best_mv[list][n];
        uint32_t bssd = ssd ? c->ssdc[pu * 9 + 8] : 0;
        int16_t  xm = me_mvx(mv), ym = me_mvy(mv);
        int      method = (ym & 2) + ((xm & 2) >> 1);
        int      dir = c->st->dir[n];
        for (int i = 0; i < 8; i++) {
            if (!me_qvalid(method != 0, dir, i)) continue;
            int sx, sy;
            me_dmv_get(i, &sx, &sy);
            if (ssd) {
                uint32_t e = c->ssdc[pu * 9 + i];
                if (e < bssd) { bssd = e; best = me_cand_get(c, pu * 8 + i); mv = me_pack_mv(xm + sx, ym + sy); }
            } else {
                uint32_t d = me_cand_get(c, pu * 8 + i);
                if (sub_sad) d <<= 1;
                if (d < best) { best = d; mv = me_pack_mv(xm + sx, ym + sy); }
            }
        }
        c->st->best_sad[list][n] = best;
        c->st->best_mv[list][n]  = mv;
        if (ssd) c->ssdc[pu * 9 + 8] = bssd;
    }
}

#ifndef SVT_HOST_EMU /* device only: ph_subpel_fast; the emulation runs ph_halfpel / ph_quarterpel and their decisions, ph_store_pred0 / ph_bipred; pinned by tests/test_gpu_me.py::test_me_presets_vs_oracle (the SUB_SAD presets) */
/* ---- half- and quarter-pel refinement of the 32x32 and 16x16 PUs in ONE phase (SUB_SAD search, the M5+ presets) ----
 * The task lists above spend nine tenths of their instructions on finding out what a task is.  Here a lane owns 16 samples of
 * one (subsampled) row of one PU for the whole refinement: waves 0-1 the four 32x32 PUs (32 lanes each: 16 rows x 2 halves),
 * waves 2-3 the sixteen 16x16 PUs (8 lanes each: one row per lane).  The lane keeps its 4 source dwords and runs through the 8
 * half-pel candidates (planes and offsets are compile-time per candidate), the lanes of a PU are summed with DPP row shifts
 * (inclusive prefix: the PU's last lane holds the totals), that lane takes the reference's decisions (pu_half_pel_refinement
 * :1076-1559: strict '<' in test order = minimum of (distortion, test index); direction by the tie order L,R,T,B,TL,TR,BL,BR)
 * and publishes them through LDS -- LDS operations of one wave execute in order, so the PU's other lanes (same wave) read them
 * back without a barrier -- and the three quarter-pel candidates around that direction follow the same way
 * (pu_quarter_pel_refinement_on_the_fly :2471-2715).  No candidate table, no atomics, no barrier inside. */
SVT_DEV void me_pred_ptrs(const me_ctx_t *c, int list, int sox, int soy, int pu, int px, int py, const uint8_t **a, const uint8_t **b, int *sa, int *sb);
SVT_DEV uint32_t me_pred_fetch(const uint8_t *a, const uint8_t *b, int offa, int offb);
SVT_DEV uint32_t me_sad16(const uint8_t *p, const uint32_t s[4]) { /* 16 samples at any byte alignment in LDS against 4 source dwords */
    const uint32_t  sh = (uint32_t)((uintptr_t)p & 3);
    const uint32_t *q  = (const uint32_t *)(p - sh);
    const uint32_t  l0 = q[0], l1 = q[1], l2 = q[2], l3 = q[3], l4 = q[4];
    uint32_t        d = svt_sad4(svt_alignbyte(l1, l0, sh), s[0], 0);
    d = svt_sad4(svt_alignbyte(l2, l1, sh), s[1], d);
    d = svt_sad4(svt_alignbyte(l3, l2, sh), s[2], d);
    return svt_sad4(svt_alignbyte(l4, l3, sh), s[3], d);
}
SVT_DEV uint32_t me_sad16_avg(const uint8_t *pa, const uint8_t *pb, const uint32_t s[4]) { /* the same against the rounded average of two planes */
    const uint32_t  sa = (uint32_t)((uintptr_t)pa & 3), sb = (uint32_t)((uintptr_t)pb & 3);
    const uint32_t *qa = (const uint32_t *)(pa - sa), *qb = (const uint32_t *)(pb - sb);
    const uint32_t  a0 = qa[0], a1 = qa[1], a2 = qa[2], a3 = qa[3], a4 = qa[4], b0 = qb[0], b1 = qb[1], b2 = qb[2], b3 = qb[3], b4 = qb[4];
    uint32_t        d = svt_sad4(svt_avg4(svt_alignbyte(a1, a0, sa), svt_alignbyte(b1, b0, sb)), s[0], 0);
    d = svt_sad4(svt_avg4(svt_alignbyte(a2, a1, sa), svt_alignbyte(b2, b1, sb)), s[1], d);
    d = svt_sad4(svt_avg4(svt_alignbyte(a3, a2, sa), svt_alignbyte(b3, b2, sb)), s[2], d);
    return svt_sad4(svt_avg4(svt_alignbyte(a4, a3, sa), svt_alignbyte(b4, b3, sb)), s[3], d);
}
/* inclusive sums over the lanes of a PU (8 lanes, or 32 = two DPP rows): exact in the PU's last lane */
SVT_DEV uint32_t me_pu_lanes_sum(uint32_t v, int big) {
    v = SVT_DPP_ADD(v, 0x111); v = SVT_DPP_ADD(v, 0x112); v = SVT_DPP_ADD(v, 0x114);
    if (big) {
        v = SVT_DPP_ADD(v, 0x118);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); /* row_bcast:15 into rows 1 and 3 */
    }
    return v;
}
SVT_DEV void ph_subpel_fast(const me_ctx_t *c, int tid, int list, int sox, int soy, int en32, int en16, int bipred, uint32_t *pr) {
    me_state_t *st = c->st;
    const int   w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63, big = w < 2;
    const int   refine = big ? en32 : en16; /* wave-uniform */
    if (!refine && !bipred) return;
    int pu, r, xo, px, py, last;
    if (big) { pu = 1 + 2 * w + (l >> 5); r = (l & 31) >> 1; xo = (l & 1) * 16; px = ((pu - 1) & 1) * 32; py = ((pu - 1) >> 1) * 32; last = (l & 31) == 31; }
    else { pu = 5 + 8 * (w - 2) + (l >> 3); r = l & 7; xo = 0; px = ((pu - 5) & 3) * 16; py = ((pu - 5) >> 2) * 16; last = (l & 7) == 7; }
    const int n = me_pu_nidx(pu), ps = c->L.plane_stride, pb = c->L.plane_bytes;
    uint32_t  s[4];
    {
        const uint32_t *sp = (const uint32_t *)(c->src + (py + 2 * r) * ME_SB + px + xo);
        s[0] = sp[0]; s[1] = sp[1]; s[2] = sp[2]; s[3] = sp[3];
    }
    uint32_t mv = st->best_mv[list][n], best = st->best_sad[list][n];
    int      xm = me_mvx(mv), ym = me_mvy(mv);
    /* ---- half-pel: 8 candidates ---- */
    if (refine) {
        const int      xs = (int16_t)((xm >> 2) - (int16_t)sox) + px + xo, ys = (int16_t)((ym >> 2) - (int16_t)soy) + py + 2 * r;
        const uint8_t *base = c->planes + ME_MUL(ys + ME_PL_G, ps) + xs + ME_PL_G; /* plane B at (xs, ys); H, J one / two planes further */
        uint32_t       d[8];
        _Pragma("unroll") for (int i = 0; i < 8; i++) {
            int hpl, hdx, hdy;
            me_hcand_get(i, &hpl, &hdx, &hdy);
            d[i] = me_sad16(base + (hpl - 1) * pb + hdy * ps + hdx, s);
        }
        /* a lane's sums stay below 2^12 and a group of 8 lanes below 2^15: two candidates per dword for the first three steps */
        uint32_t p4[4];
        _Pragma("unroll") for (int i = 0; i < 4; i++) {
            uint32_t v = d[i] | (d[i + 4] << 16);
            v = SVT_DPP_ADD(v, 0x111); v = SVT_DPP_ADD(v, 0x112); v = SVT_DPP_ADD(v, 0x114);
            p4[i] = v;
        }
        _Pragma("unroll") for (int i = 0; i < 4; i++) { d[i] = p4[i] & 0xffffu; d[i + 4] = p4[i] >> 16; }
        if (big) {
            _Pragma("unroll") for (int i = 0; i < 8; i++) {
                uint32_t v = SVT_DPP_ADD(d[i], 0x118);
                d[i] = v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
            }
        }
        /* decisions (meaningful in the PU's last lane): distortions are doubled (rows 0, 2, 4, ...) */
        uint32_t km = 0xffffffffu, kr = 0xffffffffu;
        _Pragma("unroll") for (int i = 0; i < 8; i++) {
            const uint32_t dd = d[i] << 4; /* (2 d) << 3 */
            const uint32_t k1 = dd | (uint32_t)i, k2 = dd | (uint32_t)(i == 6 ? 7 : i == 7 ? 6 : i);
            km = k1 < km ? k1 : km; kr = k2 < kr ? k2 : kr;
        }
        if ((km >> 3) < best) {
            int sx, sy;
            me_dmv_get((int)(km & 7u), &sx, &sy);
            best = km >> 3; mv = me_pack_mv(xm + 2 * sx, ym + 2 * sy);
        }
        const uint32_t dir = (0x46205137u >> (4 * (kr & 7u))) & 7u; /* tie rank L,R,T,B,TL,TR,BL,BR -> direction code */
        if (last) { st->best_sad[list][n] = best; st->best_mv[list][n] = mv; st->dir[n] = (uint8_t)dir; }
    }
    __asm__ volatile("" ::: "memory"); /* the reads below must stay behind the stores above (other lanes' data) */
    /* ---- quarter-pel: the three positions around the half-pel direction ---- */
    if (refine) {
        mv = st->best_mv[list][n]; best = st->best_sad[list][n];
        const int dir = st->dir[n];
        xm = me_mvx(mv); ym = me_mvy(mv);
        const int method = (ym & 2) + ((xm & 2) >> 1);
        const int xs = (int16_t)(((xm + 2) >> 2) - (int16_t)sox) + px + xo, ys = (int16_t)(((ym + 2) >> 2) - (int16_t)soy) + py + 2 * r;
        uint32_t  q[3], pos[3];
        _Pragma("unroll") for (int j = 0; j < 3; j++) {
            const int dirx = ((method != 0 ? dir ^ 4 : dir) + j - 1) & 7;
            pos[j] = (0x07361524u >> (4 * dirx)) & 7u; /* direction code -> L,R,T,B,TL,TR,BR,BL index */
            const uint32_t e = me_qtab_get(method, (int)pos[j]);
            const uint8_t *a = me_plane_at(c, (int)(e & 3), xs - (int)((e >> 2) & 1), ys - (int)((e >> 3) & 1));
            const uint8_t *b = me_plane_at(c, (int)((e >> 4) & 3), xs - (int)((e >> 6) & 1), ys - (int)((e >> 7) & 1));
            q[j] = me_sad16_avg(a, b, s);
        }
        uint32_t v01 = q[0] | (q[1] << 16), v2 = q[2];
        v01 = SVT_DPP_ADD(v01, 0x111); v01 = SVT_DPP_ADD(v01, 0x112); v01 = SVT_DPP_ADD(v01, 0x114);
        v2 = SVT_DPP_ADD(v2, 0x111); v2 = SVT_DPP_ADD(v2, 0x112); v2 = SVT_DPP_ADD(v2, 0x114);
        q[0] = v01 & 0xffffu; q[1] = v01 >> 16; q[2] = v2;
        if (big) {
            _Pragma("unroll") for (int j = 0; j < 3; j++) {
                uint32_t v = SVT_DPP_ADD(q[j], 0x118);
                q[j] = v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
            }
        }
        uint32_t km = 0xffffffffu;
        _Pragma("unroll") for (int j = 0; j < 3; j++) { const uint32_t k = (q[j] << 4) | pos[j]; km = k < km ? k : km; }
        if (last && (km >> 3) < best) {
            int sx, sy;
            me_dmv_get((int)(km & 7u), &sx, &sy);
            st->best_sad[list][n] = km >> 3; st->best_mv[list][n] = me_pack_mv(xm + sx, ym + sy);
        }
    }
    /* ---- the lane's 16 samples of the PU's prediction at its final motion vector (select_buffer :3310 / quarter_pel_compensation
     * :3358): kept in registers after list 0; after list 1 averaged with them and compared with the source -- the PU's
     * bi-prediction distortion (bi_pred_averging :3466-3560), summed over the PU's lanes, written by its last lane ---- */
    if (bipred) {
        __asm__ volatile("" ::: "memory");
        const uint8_t *a, *b;
        int            sa, sb;
        me_pred_ptrs(c, list, sox, soy, pu, px + xo, py + 2 * r, &a, &b, &sa, &sb);
        uint32_t v[4];
        {
            const uint32_t  sh = (uint32_t)((uintptr_t)a & 3);
            const uint32_t *q  = (const uint32_t *)(a - sh);
            const uint32_t  l0 = q[0], l1 = q[1], l2 = q[2], l3 = q[3], l4 = q[4];
            v[0] = svt_alignbyte(l1, l0, sh); v[1] = svt_alignbyte(l2, l1, sh); v[2] = svt_alignbyte(l3, l2, sh); v[3] = svt_alignbyte(l4, l3, sh);
        }
        if (b) {
            const uint32_t  sh = (uint32_t)((uintptr_t)b & 3);
            const uint32_t *q  = (const uint32_t *)(b - sh);
            const uint32_t  l0 = q[0], l1 = q[1], l2 = q[2], l3 = q[3], l4 = q[4];
            v[0] = svt_avg4(v[0], svt_alignbyte(l1, l0, sh)); v[1] = svt_avg4(v[1], svt_alignbyte(l2, l1, sh));
            v[2] = svt_avg4(v[2], svt_alignbyte(l3, l2, sh)); v[3] = svt_avg4(v[3], svt_alignbyte(l4, l3, sh));
        }
        if (list == 0) { pr[4] = v[0]; pr[5] = v[1]; pr[6] = v[2]; pr[7] = v[3]; }
        else {
            uint32_t d = svt_sad4(svt_avg4(pr[4], v[0]), s[0], 0);
            d = svt_sad4(svt_avg4(pr[5], v[1]), s[1], d);
            d = svt_sad4(svt_avg4(pr[6], v[2]), s[2], d);
            d = svt_sad4(svt_avg4(pr[7], v[3]), s[3], d);
            d = me_pu_lanes_sum(d, big);
            if (last) c->cand[pu] = d;
        }
        /* the 64x64 PU (never refined on this path: its vector is the full-pel one): every lane takes dword tid & 15 of the
         * subsampled rows 2 (tid >> 4) and 2 (tid >> 4) + 32; wave sums into cand[0], which the position-decode phase zeroed */
        const uint8_t *a0, *b0;
        int            sa0, sb0;
        me_pred_ptrs(c, list, sox, soy, 0, 0, 0, &a0, &b0, &sa0, &sb0);
        uint32_t d0 = 0;
        _Pragma("unroll") for (int k = 0; k < 2; k++) {
            const int      rr = 2 * (tid >> 4) + 32 * k, ii = tid & 15;
            const uint32_t vb = me_pred_fetch(a0, b0, ME_MUL(rr, sa0) + 4 * ii, ME_MUL(rr, sb0) + 4 * ii);
            if (list == 0) pr[k] = vb;
            else d0 = svt_sad4(svt_avg4(pr[k], vb), *(const uint32_t *)(c->src + rr * ME_SB + 4 * ii), d0);
        }
        if (list != 0) svt_wave_add_u32(&c->cand[0], d0, 1);
    }
}
#endif

/* Build the prediction block of the current list for every PU that takes part in bi-prediction
 * (select_buffer :3310 / quarter_pel_compensation :3358): task = (pu, row).  Output pred[pu_off + r*w + x].
 * Layout of pred blocks: pu 0 at 0 (64x64), 32x32 at 4096 + i*1024, 16x16 at 8192 + i*256, 8x8 at 12288 + i*64. */
SVT_DEV int me_pu_bipred(const me_ctx_t *c, int pu) {
    return (c->p->cu8x8_mode == 0 || pu < 21) && (c->p->cu16x16_mode == 0 || pu < 5);
}
/* prediction of `list` for a PU at its best mv: up to two source planes averaged (select_buffer :3310 /
 * quarter_pel_compensation :3358) */
SVT_DEV void me_pred_ptrs(const me_ctx_t *c, int list, int sox, int soy, int pu, int px, int py, const uint8_t **a, const uint8_t **b, int *sa, int *sb) {
    uint32_t mv = c->st->best_mv[list][me_pu_nidx(pu)];
    int16_t  mx = me_mvx(mv), my = me_mvy(mv);
    int      xi = (int16_t)(mx >> 2) - (int16_t)sox + px;
    int      yi = (int16_t)(my >> 2) - (int16_t)soy + py;
    int      frac = ((uint8_t)mx & 3) + (((uint8_t)my & 3) << 2);
    int            has_b;
    const uint32_t e = me_btab_get(frac, &has_b);
    *a = me_plane_at(c, (int)(e & 3), xi + (int)((e >> 2) & 1), yi + (int)((e >> 3) & 1));
    *b = has_b ? me_plane_at(c, (int)((e >> 4) & 3), xi + (int)((e >> 6) & 1), yi + (int)((e >> 7) & 1)) : 0;
    *sa = me_plane_stride(c, (int)(e & 3)); *sb = me_plane_stride(c, (int)((e >> 4) & 3));
}
SVT_DEV uint32_t me_pred_fetch(const uint8_t *a, const uint8_t *b, int offa, int offb) {
    uint32_t va = me_ld32u(a + offa);
    if (b) {
        uint32_t vb = me_ld32u(b + offb);
        va = svt_avg4(va, vb); /* (a + b + 1) >> 1 per byte */
    }
    return va;
}
SVT_DEV int me_bipred_levels(const me_ctx_t *c) { return c->p->cu16x16_mode != 0 ? 2 : c->p->cu8x8_mode != 0 ? 3 : 4; }

/* Bi-pred work split: level L (0 = 64x64 ... 3 = 8x8) has 4^L PUs of (1024 >> 2L) dwords; 256 >> 2L consecutive lanes
 * own one PU and each lane handles K dwords of it (K = 4, or 2 with SUB_SAD where only even rows count).  A lane meets
 * the same (level, k) dwords again when list 1 is searched: list 0's dword of (level, k) waits in the lane's own
 * registers pr[4 L + k] (at most 16; every index is a compile-time constant after unrolling).  The serial host
 * emulation keeps them in memory instead: ME_PR(j) = pred0[j * 256 + tid]. */
SVT_DEV void ph_store_pred0(const me_ctx_t *c, int tid, int sox, int soy, uint32_t *pr, int lmax) {
    const int sub = c->p->fractional_search_method == SVT_SUB_SAD_SEARCH, K = sub ? 2 : 4, levels = me_bipred_levels(c) < lmax ? me_bipred_levels(c) : lmax;
    _Pragma("unroll") for (int L = 0; L < 4; L++) {
        if (L >= levels) break;
        const int sh = 8 - 2 * L, l = tid & ((1 << sh) - 1), pu = (int)((0x15050100u >> (8 * L)) & 0xff) + (tid >> sh);
        int       px, py, w;
        me_pu_geom(pu, &px, &py, &w);
        const uint8_t *a, *b;
        int sa, sb;
        me_pred_ptrs(c, 0, sox, soy, pu, px, py, &a, &b, &sa, &sb);
        _Pragma("unroll") for (int k = 0; k < 4; k++) {
            if (k < K) {
                int d = l + (k << sh), r = (d >> (4 - L)) << sub, i = d & ((16 >> L) - 1);
                ME_PR(4 * L + k) = me_pred_fetch(a, b, ME_MUL(r, sa) + 4 * i, ME_MUL(r, sb) + 4 * i);
            }
        }
        SVT_SCHED_FENCE();
    }
}
/* bi-pred distortion: avg-SAD of (list0 pred, list1 pred) vs source (bi_pred_averging :3466-3560) */
SVT_DEV void ph_bipred(const me_ctx_t *c, int tid, int sox, int soy, const uint32_t *pr, int lmax) {
    const int sub = c->p->fractional_search_method == SVT_SUB_SAD_SEARCH, K = sub ? 2 : 4, levels = me_bipred_levels(c) < lmax ? me_bipred_levels(c) : lmax;
    _Pragma("unroll") for (int L = 0; L < 4; L++) {
        if (L >= levels) break;
        const int sh = 8 - 2 * L, l = tid & ((1 << sh) - 1), pu = (int)((0x15050100u >> (8 * L)) & 0xff) + (tid >> sh);
        int       px, py, w;
        me_pu_geom(pu, &px, &py, &w);
        const uint8_t *a, *b;
        int sa, sb;
        me_pred_ptrs(c, 1, sox, soy, pu, px, py, &a, &b, &sa, &sb);
        uint32_t dsum = 0;
        _Pragma("unroll") for (int k = 0; k < 4; k++) {
            if (k < K) {
                int      d = l + (k << sh), r = (d >> (4 - L)) << sub, i = d & ((16 >> L) - 1);
                uint32_t s  = *(const uint32_t *)(c->src + (py + r) * ME_SB + px + 4 * i);
                uint32_t va = ME_PR(4 * L + k), vb = me_pred_fetch(a, b, ME_MUL(r, sa) + 4 * i, ME_MUL(r, sb) + 4 * i);
                uint32_t av = svt_avg4(va, vb);
                dsum = svt_sad4(av, s, dsum);
            }
        }
        svt_group_add_u32(&c->cand[pu], dsum, sh > 6 ? 64 : 1 << sh);
        SVT_SCHED_FENCE();
    }
}

#endif
