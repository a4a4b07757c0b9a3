/* me_hme.h -- the hierarchical search (hme_level0/1/2): one thread (or four lanes) plans a level into a work list of windows in LDS,
 * the workgroup loads and searches them batch by batch, the results are scaled and the centre chosen. */
#ifndef SVT_ME_HME_H
#define SVT_ME_HME_H
#include "me_types.h"
#include "me_prof.h"

/* copy the windows [e0, e1) of a batch: flattened (window, row, 16-byte unit) tasks -- one global load per unit (the last unit
 * of a row is shortened to whole dwords), two units in flight per thread before the LDS stores; ntask = total load tasks */
#define ME_HME_UNITS(nd) (((nd) + 3) >> 2)
SVT_DEV void ph_hme_load_multi(const me_ctx_t *c, int tid, const svt_plane *ref_lds, const me_hme_win *wn, int e0, int e1, int ntask) {
    const svt_plane  ref_u = me_plane_uni(ref_lds);
    const svt_plane *ref = &ref_u;
    for (int t0 = tid; t0 < ntask; t0 += 2 * SVT_NT) {
        me_u32x4 v[2];
        int      dst[2], k[2];
        _Pragma("unroll") for (int u = 0; u < 2; u++) {
            int T = t0 + u * SVT_NT;
            dst[u] = -1; k[u] = 0;
            if (T < ntask) {
                int e = e0;
                while (e + 1 < e1 && T >= wn[e + 1].tl) e++;
                const int t = T - wn[e].tl, nd = wn[e].nd, nu = ME_HME_UNITS(nd);
                const int row = me_div_magic(t, wn[e].inv_nu), i = t - row * nu;
                const uint8_t *gp = me_pix(ref, wn[e].gx + 16 * i, wn[e].gy + row);
                k[u] = nd - 4 * i < 4 ? nd - 4 * i : 4;
                if (k[u] == 4) v[u] = me_ld128u_g(gp);
                else {
                    v[u].x = me_ld32u_g(gp);
                    v[u].y = k[u] > 1 ? me_ld32u_g(gp + 4) : 0;
                    v[u].z = k[u] > 2 ? me_ld32u_g(gp + 8) : 0;
                    v[u].w = 0;
                }
                dst[u] = wn[e].off + row * wn[e].wstride + 16 * i;
            }
        }
        _Pragma("unroll") for (int u = 0; u < 2; u++)
            if (dst[u] >= 0) {
                uint32_t *d = (uint32_t *)(c->hme_scratch + dst[u]);
                d[0] = v[u].x;
                if (k[u] > 1) d[1] = v[u].y;
                if (k[u] > 2) d[2] = v[u].z;
                if (k[u] > 3) d[3] = v[u].w;
            }
    }
}

/* SADs of 4 consecutive search positions (window dwords wr..) against a bw x bh block; window row of block row j is
 * mul*j rows further down.  The packed u16 accumulators are flushed before they can overflow.  Two block rows are
 * processed per step with independent accumulators and all their LDS loads issued up front: the QSAD chain of one
 * row overlaps the other's (a dependent v_qsad_pk_u16_u8 costs ~26 cycles, an LDS round trip ~64+). */
SVT_DEV void me_qsad_row4(const uint32_t *wr, const uint32_t *br, uint64_t *acc) {
    const uint32_t w0 = wr[0], w1 = wr[1], w2 = wr[2], w3 = wr[3], w4 = wr[4];
    const uint32_t b0 = br[0], b1 = br[1], b2 = br[2], b3 = br[3];
    uint64_t       a = *acc;
    a = svt_qsad(((uint64_t)w1 << 32) | w0, b0, a);
    a = svt_qsad(((uint64_t)w2 << 32) | w1, b1, a);
    a = svt_qsad(((uint64_t)w3 << 32) | w2, b2, a);
    a = svt_qsad(((uint64_t)w4 << 32) | w3, b3, a);
    *acc = a;
}
SVT_DEV void me_qsad_block(const uint8_t *blk, int bstride, int nd, int bh, const uint8_t *win, int wstride, int mul, uint32_t a[4]) {
    /* rows whose sums (4*nd*255 each) still fit 16 bits.  The even / odd accumulators below hold flush/2 rows each, so the bound has a factor
     * of two of slack (twice the rows still fit); four times does not: 16 rows of 64 samples carry into the neighbouring field, at the ceiling
     * only (tests/test_me_ceiling.py) */
    const int flush = nd <= 4 ? 16 : nd <= 8 ? 8 : 4;
    a[0] = a[1] = a[2] = a[3] = 0;
    for (int j0 = 0; j0 < bh; j0 += flush) {
        uint64_t  acc0 = 0, acc1 = 0; /* even / odd rows of the group: each holds at most flush/2 rows */
        const int j1  = j0 + flush < bh ? j0 + flush : bh;
        int       j   = j0;
        if (nd == 4) { /* 16-sample rows (1/16-resolution level): the whole row pair is loaded before the first QSAD */
            for (; j + 2 <= j1; j += 2) {
                const uint32_t *wa = (const uint32_t *)(win + mul * j * wstride), *wb = (const uint32_t *)(win + mul * (j + 1) * wstride);
                const uint32_t *ba = (const uint32_t *)(blk + j * bstride), *bb = (const uint32_t *)(blk + (j + 1) * bstride);
                const uint32_t  x0 = wa[0], x1 = wa[1], x2 = wa[2], x3 = wa[3], x4 = wa[4];
                const uint32_t  y0 = wb[0], y1 = wb[1], y2 = wb[2], y3 = wb[3], y4 = wb[4];
                const uint32_t  p0 = ba[0], p1 = ba[1], p2 = ba[2], p3 = ba[3], q0 = bb[0], q1 = bb[1], q2 = bb[2], q3 = bb[3];
                acc0 = svt_qsad(((uint64_t)x1 << 32) | x0, p0, acc0); acc1 = svt_qsad(((uint64_t)y1 << 32) | y0, q0, acc1);
                acc0 = svt_qsad(((uint64_t)x2 << 32) | x1, p1, acc0); acc1 = svt_qsad(((uint64_t)y2 << 32) | y1, q1, acc1);
                acc0 = svt_qsad(((uint64_t)x3 << 32) | x2, p2, acc0); acc1 = svt_qsad(((uint64_t)y3 << 32) | y2, q2, acc1);
                acc0 = svt_qsad(((uint64_t)x4 << 32) | x3, p3, acc0); acc1 = svt_qsad(((uint64_t)y4 << 32) | y3, q3, acc1);
            }
        }
        for (; j < j1; j++) {
            const uint32_t *wr = (const uint32_t *)(win + mul * j * wstride);
            const uint32_t *br = (const uint32_t *)(blk + j * bstride);
            uint64_t        acc = (j & 1) ? acc1 : acc0;
            int             i = 0;
            for (; i + 4 <= nd; i += 4) me_qsad_row4(wr + i, br + i, &acc);
            if (i < nd) {
                uint32_t lo = wr[i];
                for (; i < nd; i++) {
                    uint32_t hi = wr[i + 1];
                    acc         = svt_qsad(((uint64_t)hi << 32) | lo, br[i], acc);
                    lo          = hi;
                }
            }
            if (j & 1) acc1 = acc; else acc0 = acc;
        }
        a[0] += (uint32_t)(acc0 & 0xffff) + (uint32_t)(acc1 & 0xffff);
        a[1] += (uint32_t)((acc0 >> 16) & 0xffff) + (uint32_t)((acc1 >> 16) & 0xffff);
        a[2] += (uint32_t)((acc0 >> 32) & 0xffff) + (uint32_t)((acc1 >> 32) & 0xffff);
        a[3] += (uint32_t)(acc0 >> 48) + (uint32_t)(acc1 >> 48);
    }
}


/* the 1/16-resolution level with a whole SB (16 x 8 block, rows of 4 dwords; window rows two apart): straight-line task --
 * each QSAD operand pair is read as such (the overlapping pairs cost LDS reads, not register moves), one packed add joins the
 * even / odd row accumulators (8 rows x 16 samples x 255 < 2^16) */
SVT_DEV void me_qsad_16x8(const uint8_t *blk, const uint8_t *win, int wstride, uint32_t *lo_out, uint32_t *hi_out) {
    uint64_t acc0 = 0, acc1 = 0;
    _Pragma("unroll") for (int j = 0; j < 8; j++) {
        const uint32_t *w = (const uint32_t *)(win + 2 * j * wstride), *b = (const uint32_t *)(blk + 16 * j);
        uint64_t        a = (j & 1) ? acc1 : acc0;
        _Pragma("unroll") for (int i = 0; i < 4; i++) a = svt_qsad(((uint64_t)w[i + 1] << 32) | w[i], b[i], a);
        if (j & 1) acc1 = a; else acc0 = a;
    }
    *lo_out = (uint32_t)acc0 + (uint32_t)acc1;                 /* positions 0, 1 as 16-bit sums: no carry between the halves */
    *hi_out = (uint32_t)(acc0 >> 32) + (uint32_t)(acc1 >> 32); /* positions 2, 3 */
}

/* exhaustive search of the windows [e0, e1) of a batch in one phase; keys[slot] = min over
 * (sad << 32 | y << 16 | x inside the region): ordered like the raster index, no division to take it apart */
#ifndef SVT_HOST_EMU /* device only: the windows of a batch in scalar registers; the emulation finds a task's window by walking the work list in LDS; pinned by tests/test_gpu_me.py::test_me_presets_vs_oracle */
/* The windows of a batch (at most four here: one per region, or the bands of one), held in scalar registers: a task finds its window
 * by three comparisons instead of walking the list in LDS -- every task used to start with up to five dependent LDS round trips
 * (~120 cycles each with one wave per SIMD) before its first sample was fetched. */
typedef struct me_hme_sel { int ts[4], sw[4], slot[4], y0[4], ws[4], off[4]; uint32_t inv[4]; } me_hme_sel;
SVT_DEV void me_hme_sel_load(me_hme_sel *S, const me_hme_win *wn, int e0, int e1) {
    _Pragma("unroll") for (int k = 0; k < 4; k++) {
        const me_hme_win *w = &wn[e0 + k < e1 ? e0 + k : e1 - 1];
        S->ts[k] = e0 + k < e1 ? ME_UNI(w->ts) : 0x7fffffff;
        S->sw[k] = ME_UNI(w->sw); S->slot[k] = ME_UNI(w->slot); S->y0[k] = ME_UNI(w->y0); S->ws[k] = ME_UNI(w->wstride);
        S->off[k] = ME_UNI(w->off); S->inv[k] = (uint32_t)ME_UNI(w->inv_ng);
    }
}
#define ME_HME_SEL(S, T, f) ((T) >= (S).ts[3] ? (S).f[3] : (T) >= (S).ts[2] ? (S).f[2] : (T) >= (S).ts[1] ? (S).f[1] : (S).f[0])
#endif
SVT_DEV void ph_hme_search_multi(const me_ctx_t *c, int tid, const uint8_t *blk, int bstride, int bw, int bh, const me_hme_win *wn,
                                 int e0, int e1, int ntask, uint64_t *keys, int slot_mask) {
    const int qs = (bw & 3) == 0; /* QSAD path: task = 4 positions */
    uint64_t  best[4] = {~0ull, ~0ull, ~0ull, ~0ull}; /* per key slot */
    int       cur = -1;
    uint32_t  inv = 0;
    ME_FINE_BEGIN();
    if (bw == 16 && bh == 8 && bstride == 16 && c->L.hme_tw0 <= 256 && c->L.hme_th0 <= 256 && c->L.hme_w0[0] <= 256 && c->L.hme_w0[1] <= 256 &&
        c->L.hme_h0[0] <= 256 && c->L.hme_h0[1] <= 256) { /* positions inside a region fit 8 bits each */
        uint32_t b32[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
#ifndef SVT_HOST_EMU /* device only: window lookup through me_hme_sel; the emulation walks the work list (the braces in the loop); pinned by tests/test_gpu_me.py::test_me_presets_vs_oracle */
        me_hme_sel S;
        const bool sel = e1 - e0 <= 4;
        if (sel) me_hme_sel_load(&S, wn, e0, e1);
#endif
        for (int T = tid; T < ntask; T += SVT_NT) {
            int      t, sw, slot, w_y0, w_ws, w_off;
            uint32_t w_inv;
#ifndef SVT_HOST_EMU /* device only: window lookup through me_hme_sel; the emulation takes the braces below; pinned by tests/test_gpu_me.py::test_me_presets_vs_oracle */
            if (sel) {
                t = T - ME_HME_SEL(S, T, ts); sw = ME_HME_SEL(S, T, sw); slot = ME_HME_SEL(S, T, slot); w_y0 = ME_HME_SEL(S, T, y0);
                w_ws = ME_HME_SEL(S, T, ws); w_off = ME_HME_SEL(S, T, off); w_inv = ME_HME_SEL(S, T, inv);
            } else
#endif
            {
                int e = e0;
                while (e + 1 < e1 && T >= wn[e + 1].ts) e++;
                t = T - wn[e].ts; sw = wn[e].sw; slot = wn[e].slot; w_y0 = wn[e].y0; w_ws = wn[e].wstride; w_off = (int)wn[e].off; w_inv = wn[e].inv_ng;
            }
            const int ng = (sw + 3) >> 2, y = me_div_magic(t, w_inv), g = t - ME_MUL(y, ng);
            uint32_t  lo, hi;
            me_qsad_16x8(blk, c->hme_scratch + w_off + ME_MUL(y, w_ws) + 4 * g, w_ws, &lo, &hi);
            const uint32_t pos = ((uint32_t)(w_y0 + y) << 8) | (uint32_t)(4 * g);
            uint32_t       k0 = (lo << 16) | pos, k1 = (lo & 0xffff0000u) | (pos + 1), k2 = (hi << 16) | (pos + 2), k3 = (hi & 0xffff0000u) | (pos + 3);
            if (4 * g + 3 >= sw) { /* last group of a width that is not a multiple of 4 */
                if (4 * g + 1 >= sw) k1 = 0xffffffffu;
                if (4 * g + 2 >= sw) k2 = 0xffffffffu;
                k3 = 0xffffffffu;
            }
            k0 = k0 < k1 ? k0 : k1; k2 = k2 < k3 ? k2 : k3; k0 = k0 < k2 ? k0 : k2;
            _Pragma("unroll") for (int q = 0; q < 4; q++) if (q == slot && k0 < b32[q]) b32[q] = k0;
        }
        _Pragma("unroll") for (int q = 0; q < 4; q++) if ((slot_mask >> q) & 1) svt_wave_min_key32(&keys[q], b32[q]);
        return;
    }
#ifndef SVT_HOST_EMU /* device only: 8 / 16 lanes share a task of the 1/4- and full-resolution levels; the emulation runs the generic loop behind it; pinned by tests/test_gpu_me.py::test_me_presets_vs_oracle and ::test_me_c5_ssd_search_vs_oracle */
    if (qs && (bw == 32 || bw == 64) && (bh == 16 || bh == 32)) {
        /* The quarter- and full-resolution levels of a whole SB: few tasks (a region is 4 x 2 .. 16 x 16 positions) of many samples each
         * (32 x 16 / 64 x 32 rows) -- one lane per task left three waves idle while a handful of lanes walked 128 / 512 QSADs each (the
         * 1080p presets: 8 lanes busy for ~20 K cycles).  Here bw / 4 = 8 or 16 neighbouring lanes share a task: a lane owns one dword
         * column of the block over all its rows (4 positions x <= 32 rows x 4 samples x 255 stay below 2^16 per 16-bit sum), the
         * columns meet in DPP row shifts (the group's last lane holds the four sums), and that lane keeps the task's key. */
        const int lsh = bw == 64 ? 4 : 3, nl = 1 << lsh, sub = tid & (nl - 1), tpp = SVT_NT >> lsh;
        const uint8_t *bcol = blk + 4 * sub;
        me_hme_sel     S;
        const bool     sel = e1 - e0 <= 4;
        if (sel) me_hme_sel_load(&S, wn, e0, e1);
        for (int T0 = 0; T0 < ntask; T0 += tpp) {
            const int  T = T0 + (tid >> lsh);
            const bool act = T < ntask;
            int        a0 = 0, a1 = 0, a2 = 0, a3 = 0, slot = 0, sw = 0, y = 0, g = 0, y0 = 0;
            if (act) {
                int      t, ws, w_off;
                uint32_t w_inv;
                if (sel) {
                    t = T - ME_HME_SEL(S, T, ts); sw = ME_HME_SEL(S, T, sw); slot = ME_HME_SEL(S, T, slot); y0 = ME_HME_SEL(S, T, y0);
                    ws = ME_HME_SEL(S, T, ws); w_off = ME_HME_SEL(S, T, off); w_inv = ME_HME_SEL(S, T, inv);
                } else {
                    int e = e0;
                    while (e + 1 < e1 && T >= wn[e + 1].ts) e++;
                    t = T - wn[e].ts; ws = wn[e].wstride; w_off = (int)wn[e].off; w_inv = wn[e].inv_ng;
                    sw = wn[e].sw; slot = wn[e].slot; y0 = wn[e].y0;
                }
                const int ng = (sw + 3) >> 2;
                y = me_div_magic(t, w_inv); g = t - ME_MUL(y, ng);
                const uint8_t *wp = c->hme_scratch + w_off + ME_MUL(y, ws) + 4 * g + 4 * sub;
                uint64_t       acc = 0, acc_b = 0; /* two chains; eight rows' operands are fetched before their QSADs (bh is 16 or 32) */
                const int      ws2 = 2 * ws;
                for (int j = 0; j < bh; j += 8) {
                    uint64_t pr[8];
                    uint32_t bd[8];
                    _Pragma("unroll") for (int u = 0; u < 8; u++) {
                        pr[u] = *(const me_u64a4 *)(wp + ME_MUL(j + u, ws2));
                        bd[u] = *(const uint32_t *)(bcol + ME_MUL(j + u, bstride));
                    }
                    _Pragma("unroll") for (int u = 0; u < 8; u += 2) { acc = svt_qsad(pr[u], bd[u], acc); acc_b = svt_qsad(pr[u + 1], bd[u + 1], acc_b); }
                }
                acc += acc_b; /* (16-bit sums of 32 rows x 4 samples: no carry between the fields) */
                a0 = (int)(acc & 0xffffu); a1 = (int)((acc >> 16) & 0xffffu); a2 = (int)((acc >> 32) & 0xffffu); a3 = (int)(acc >> 48);
            }
            /* every lane takes part (lanes without a task add 0); row_shr:n with bound_ctrl: lanes shifted in from outside the row read 0 */
#define HW_SHR(v, n) v += __builtin_amdgcn_update_dpp(0, v, 0x110 + (n), 0xf, 0xf, true)
            HW_SHR(a0, 1); HW_SHR(a1, 1); HW_SHR(a2, 1); HW_SHR(a3, 1);
            HW_SHR(a0, 2); HW_SHR(a1, 2); HW_SHR(a2, 2); HW_SHR(a3, 2);
            HW_SHR(a0, 4); HW_SHR(a1, 4); HW_SHR(a2, 4); HW_SHR(a3, 4);
            if (lsh == 4) { HW_SHR(a0, 8); HW_SHR(a1, 8); HW_SHR(a2, 8); HW_SHR(a3, 8); }
#undef HW_SHR
            if (act && sub == nl - 1) {
                const uint32_t av[4] = {(uint32_t)a0, (uint32_t)a1, (uint32_t)a2, (uint32_t)a3};
                uint64_t       kb = ~0ull;
                _Pragma("unroll") for (int o = 0; o < 4; o++) {
                    const int x = 4 * g + o;
                    if (x < sw) {
                        const uint64_t k = ((uint64_t)av[o] << 32) | ((uint32_t)(y0 + y) << 16) | (uint32_t)x;
                        if (k < kb) kb = k;
                    }
                }
                _Pragma("unroll") for (int q = 0; q < 4; q++) if (q == slot && kb < best[q]) best[q] = kb;
            }
        }
        _Pragma("unroll") for (int q = 0; q < 4; q++) if ((slot_mask >> q) & 1) svt_wave_min_u64(&keys[q], best[q]);
        return;
    }
#endif
    for (int T = tid; T < ntask; T += SVT_NT) {
        int e = e0;
        while (e + 1 < e1 && T >= wn[e + 1].ts) e++;
        const int      t = T - wn[e].ts, ws = wn[e].wstride, sw = wn[e].sw, slot = wn[e].slot, y0 = wn[e].y0;
        if (e != cur) { cur = e; inv = wn[e].inv_ng; }
        const uint8_t *win = c->hme_scratch + wn[e].off;
        uint64_t       kb = ~0ull;
        ME_FINE(16);
        if (qs) {
            const int ng = (sw + 3) >> 2;
            const int y = me_div_magic(t, inv), g = t - y * ng;
            uint32_t  a[4];
            me_qsad_block(blk, bstride, bw >> 2, bh, win + y * ws + 4 * g, ws, 2, a);
            ME_FINE(17);
            _Pragma("unroll") for (int o = 0; o < 4; o++) {
                int x = 4 * g + o;
                if (x < sw) {
                    uint64_t k = ((uint64_t)a[o] << 32) | ((uint32_t)(y0 + y) << 16) | (uint32_t)x;
                    if (k < kb) kb = k;
                }
            }
        } else {
            const int y = me_div_magic(t, inv), x = t - y * sw;
            uint32_t  sd = 0;
            for (int j = 0; j < bh; j++)
                for (int i = 0; i < bw; i++) {
                    int p0 = blk[j * bstride + i], p1 = win[(y + 2 * j) * ws + x + i];
                    sd += (uint32_t)(p0 > p1 ? p0 - p1 : p1 - p0);
                }
            kb = ((uint64_t)sd << 32) | ((uint32_t)(y0 + y) << 16) | (uint32_t)x;
        }
        _Pragma("unroll") for (int q = 0; q < 4; q++) if (q == slot && kb < best[q]) best[q] = kb;
        ME_FINE(18);
    }
    /* every lane takes part in the wave reductions of the slots this batch touches (lanes without work contribute ~0) */
    _Pragma("unroll") for (int q = 0; q < 4; q++) if ((slot_mask >> q) & 1) svt_wave_min_u64(&keys[q], best[q]);
    ME_FINE(19);
}

typedef struct me_hme_geom {
    const svt_plane *ref;
    const uint8_t   *blk; /* LDS */
    int              bstride, bw, bh, ox, oy, pad_w, pad_h, ref_w, ref_h;
} me_hme_geom;

SVT_DEV int16_t me_hme_round_w(int16_t w) { return (int16_t)((w < 8) ? 8 : (w & 7) ? w + (w - ((w >> 3) << 3)) : w); }

/* geometry of an HME level for one reference list (hme_level0/1/2 of Codec/EbMotionEstimation.c) */
SVT_DEV void me_hme_geom_of(const me_ctx_t *c, int list, int lvl, me_hme_geom *g) {
    if (lvl == 0) {
        g->ref = &c->st->refd[2]; g->blk = c->st->sixteenth_sb; g->bstride = 16; g->bw = c->sb_w >> 2; g->bh = (c->sb_h >> 2) >> 1;
        g->ox = (int16_t)(c->sb_x >> 2); g->oy = (int16_t)(c->sb_y >> 2);
    } else if (lvl == 1) {
        g->ref = &c->st->refd[1]; g->blk = c->quarter_sb; g->bstride = 64; g->bw = c->sb_w >> 1; g->bh = (c->sb_h >> 1) >> 1;
        g->ox = (int16_t)(c->sb_x >> 1); g->oy = (int16_t)(c->sb_y >> 1);
    } else {
        g->ref = &c->st->refd[0]; g->blk = c->src; g->bstride = 2 * ME_SB; g->bw = c->sb_w; g->bh = c->sb_h >> 1;
        g->ox = (int16_t)c->sb_x; g->oy = (int16_t)c->sb_y;
    }
    g->pad_w = lvl == 2 ? ME_SB - 1 : ME_PLAN_RD(g->ref->origin_x) - 1;
    g->pad_h = lvl == 2 ? ME_SB - 1 : ME_PLAN_RD(g->ref->origin_y) - 1;
    g->ref_w = ME_PLAN_RD(g->ref->width); g->ref_h = ME_PLAN_RD(g->ref->height);
}

/* Plan one HME level (run by ONE thread): place the search areas of the level's regions (slot = rh*2 + rw), clip them,
 * and cut them into the work list of (region, band of search rows) windows.  Consecutive windows that fit the scratch
 * together form a batch = one global-load phase + one search phase; a region too tall for the scratch is split into
 * bands -- the 64-bit key carries the raster index inside the region, so the minimum over all bands is exactly the
 * reference's first minimum in raster order.  [quirk] region-row counter semantics: see me_sb_run. */
SVT_DEV void me_hme_plan_level(const me_ctx_t *c, int list, int lvl, int16_t xsc, int16_t ysc, int first) {
    const svt_me_params *p  = c->p;
    me_state_t          *st = c->st;
    const int            NW = p->number_hme_search_region_in_width, NH = p->number_hme_search_region_in_height;
    me_hme_geom          g;
    me_hme_geom_of(c, list, lvl, &g);
    const int single = lvl == 0 && p->single_hme_quadrant && !p->enable_hme_level_1_flag && !p->enable_hme_level_2_flag;
    const int span   = 2 * (g.bh - 1);
    int       ne = 0, nb = 0, bytes = 0, tl = 0, ts = 0;
#ifndef SVT_HOST_EMU /* device only: short plan for one region at level 0; the emulation runs the general code below with k = 0; pinned by tests/test_gpu_me_ceiling.py::test_me_generic_instance_at_the_ceiling_same_pictures */
    if (single) {
        /* one region, one level (the 4K presets M8+): only slot 0 of level 0 is ever read back (me_hme_finish_level / me_hme_select
         * skip the other slots) -- the same steps as the general code below for k = 0, without the loops around them */
        st->hme_x[0][0] = (int16_t)(xsc >> 2); st->hme_y[0][0] = (int16_t)(ysc >> 2);
        st->hme_rh = 0;
        st->hme_bstart[0] = 0;
        { uint32_t *kw_ = (uint32_t *)&st->hme_keys[0]; kw_[0] = ~0u; kw_[1] = ~0u; }
        int16_t w = c->L.hme_tw0, h = c->L.hme_th0;
        int16_t ox = (int16_t)(-(int16_t)(w >> 1) + (int16_t)(xsc >> 2)), oy = (int16_t)(-(int16_t)(h >> 1) + (int16_t)(ysc >> 2));
        me_clip_area(g.ox, &ox, &w, g.pad_w, g.ref_w);
        me_clip_area(g.oy, &oy, &h, g.pad_h, g.ref_h);
        if ((w & 15) != 0) w = (int16_t)((w >> 4) << 4);
        st->hme_cox[0] = ox; st->hme_coy[0] = oy;
        const int ok = w > 0 && h > 0;
        st->hme_cw[0] = ok ? w : 0; st->hme_ch[0] = ok ? h : 0;
        if (ok) {
            const int wbytes = w + g.bw + 3;
            int       ws     = ((wbytes + 3) & ~3) + 4;
            if (((ws >> 2) & 1) == 0) ws += 4;
            const int ng = (g.bw & 3) == 0 ? (w + 3) >> 2 : w;
            for (int y = 0; y < h && ne < ME_HME_MAX_WIN;) {
                int nr = h - y;
                if (ws * (nr + span) > c->hme_scratch_bytes - bytes) nr = (c->hme_scratch_bytes - bytes) / ws - span;
                if (nr < 1 && bytes > 0) { st->hme_bstart[++nb] = ne; bytes = 0; tl = 0; ts = 0; continue; }
                if (nr < 1) break;
                me_hme_win *wn = &st->hme_win[ne++];
                wn->off = bytes; wn->wstride = ws; wn->nd = (wbytes + 3) >> 2; wn->rows = nr + span; wn->sw = w; wn->sh = nr;
                wn->gx = g.ox + ox; wn->gy = g.oy + oy + y; wn->slot = 0; wn->y0 = y; wn->tl = tl; wn->ts = ts;
                wn->inv_nu = me_magic_small(ME_HME_UNITS(wn->nd)); wn->inv_ng = me_magic_small(ng);
                tl += ME_HME_UNITS(wn->nd) * wn->rows; ts += ng * nr;
                bytes += ws * (nr + span); y += nr;
            }
        }
        if (ne > st->hme_bstart[nb]) st->hme_bstart[++nb] = ne;
        st->hme_nbatch = nb;
        return;
    }
#endif
    if (first && ME_PLAN_RD(st->hme_rh) < NH) { /* [quirk] centres are only initialised while the reference's row counter is below NH */
        for (int k = 0; k < 4; k++)
            if ((k & 1) < NW && (k >> 1) < NH && (k >> 1) >= ME_PLAN_RD(st->hme_rh)) {
                st->hme_x[0][k] = (int16_t)(xsc >> 2); st->hme_y[0][k] = (int16_t)(ysc >> 2);
                st->hme_x[1][k] = (int16_t)(xsc >> 1); st->hme_y[1][k] = (int16_t)(ysc >> 1);
                st->hme_x[2][k] = xsc; st->hme_y[2][k] = ysc;
            }
        st->hme_rh = NH;
    }
    st->hme_rh = single ? 0 : NH;
    st->hme_bstart[0] = 0;
    for (int k = 0; k < 4; k++) {
        const int rw = k & 1, rh = k >> 1;
        {   /* written as two dwords: as a 64-bit constant the compiler hoists the pair out of the SB's whole life and spills it */
            uint32_t *kw_ = (uint32_t *)&st->hme_keys[k];
            kw_[0] = ~0u; kw_[1] = ~0u;
        }
        st->hme_cw[k] = 0; st->hme_ch[k] = 0; st->hme_cox[k] = 0; st->hme_coy[k] = 0;
        if (single ? k != 0 : (rw >= NW || rh >= NH)) continue;
        int16_t w, h, ox, oy;
        if (lvl == 0) {
            /* c->L.hme_* = (area * multiplier) / 100 of hme_level0 / single_hme_quadrant_level0 (:2717-2760, 2872-2920) */
            if (single) {
                w  = c->L.hme_tw0;
                h  = c->L.hme_th0;
                ox = (int16_t)(-(int16_t)(w >> 1) + (int16_t)(xsc >> 2));
                oy = (int16_t)(-(int16_t)(h >> 1) + (int16_t)(ysc >> 2));
            } else {
                w = c->L.hme_w0[rw];
                h = c->L.hme_h0[rh];
                int16_t ddx = (int16_t)(xsc >> 2), ddy = (int16_t)(ysc >> 2);
                if (rw > 0) ddx = (int16_t)(ddx + c->L.hme_w0[0]);
                if (rh > 0) ddy = (int16_t)(ddy + c->L.hme_h0[0]);
                ox = (int16_t)(-(int16_t)(c->L.hme_tw0 >> 1) + ddx);
                oy = (int16_t)(-(int16_t)(c->L.hme_th0 >> 1) + ddy);
            }
        } else if (lvl == 1) {
            w  = me_hme_round_w((int16_t)p->hme_level1_search_area_in_width_array[rw]);
            h  = (int16_t)p->hme_level1_search_area_in_height_array[rh];
            ox = (int16_t)(-(w >> 1) + (int16_t)((int16_t)ME_PLAN_RD(st->hme_x[0][k]) >> 1));
            oy = (int16_t)(-(h >> 1) + (int16_t)((int16_t)ME_PLAN_RD(st->hme_y[0][k]) >> 1));
        } else {
            w  = me_hme_round_w((int16_t)p->hme_level2_search_area_in_width_array[rw]);
            h  = (int16_t)p->hme_level2_search_area_in_height_array[rh];
            ox = (int16_t)(-(w >> 1) + (int16_t)ME_PLAN_RD(st->hme_x[1][k]));
            oy = (int16_t)(-(h >> 1) + (int16_t)ME_PLAN_RD(st->hme_y[1][k]));
        }
        me_clip_area(g.ox, &ox, &w, g.pad_w, g.ref_w);
        me_clip_area(g.oy, &oy, &h, g.pad_h, g.ref_h);
        if (single && (w & 15) != 0) w = (int16_t)((w >> 4) << 4);
        st->hme_cox[k] = ox; st->hme_coy[k] = oy; /* kept even when nothing is searched: the centre still moves by them */
        if (w <= 0 || h <= 0) continue;
        st->hme_cw[k] = w; st->hme_ch[k] = h;
        const int wbytes = w + g.bw + 3;
        int       ws     = ((wbytes + 3) & ~3) + 4;
        if (((ws >> 2) & 1) == 0) ws += 4;
        const int ng = (g.bw & 3) == 0 ? (w + 3) >> 2 : w;
        for (int y = 0; y < h && ne < ME_HME_MAX_WIN;) {
            /* search rows that still fit the scratch: usually all of them -- the division only runs otherwise */
            int nr = h - y;
            if (ws * (nr + span) > c->hme_scratch_bytes - bytes) nr = (c->hme_scratch_bytes - bytes) / ws - span;
            if (nr < 1 && bytes > 0) { /* close the batch and retry with an empty scratch */
                st->hme_bstart[++nb] = ne; bytes = 0; tl = 0; ts = 0;
                continue;
            }
            if (nr < 1) break; /* cannot happen with the scratch sizes of me_lds_layout_compute */
            me_hme_win *wn = &st->hme_win[ne++];
            wn->off = bytes; wn->wstride = ws; wn->nd = (wbytes + 3) >> 2; wn->rows = nr + span; wn->sw = w; wn->sh = nr;
            wn->gx = g.ox + ox; wn->gy = g.oy + oy + y; wn->slot = k; wn->y0 = y; wn->tl = tl; wn->ts = ts;
            wn->inv_nu = me_magic_small(ME_HME_UNITS(wn->nd)); wn->inv_ng = me_magic_small(ng);
            tl += ME_HME_UNITS(wn->nd) * wn->rows; ts += ng * nr;
            bytes += ws * (nr + span); y += nr;
        }
    }
    if (ne > st->hme_bstart[nb]) st->hme_bstart[++nb] = ne;
    st->hme_nbatch = nb;
}

/* results of one HME level (run by ONE thread): position scaling and SAD*2 as in hme_level0/1/2 */
SVT_DEV void me_hme_finish_level(const me_ctx_t *c, int lvl) {
    const svt_me_params *p  = c->p;
    me_state_t          *st = c->st;
    const int            NW = p->number_hme_search_region_in_width, NH = p->number_hme_search_region_in_height;
    const int single = lvl == 0 && p->single_hme_quadrant && !p->enable_hme_level_1_flag && !p->enable_hme_level_2_flag;
    const int scale  = 4 >> lvl;
    for (int k = 0; k < 4; k++) {
        if (single ? k != 0 : ((k & 1) >= NW || (k >> 1) >= NH)) continue;
        uint64_t sad = 0xffffff;
        int16_t  x = (int16_t)ME_PLAN_RD(st->hme_x[lvl][k]), y = (int16_t)ME_PLAN_RD(st->hme_y[lvl][k]);
        if (st->hme_cw[k] > 0) {
            const uint64_t key = st->hme_keys[k];
            if (key != ~0ull) {
                const uint32_t idx = (uint32_t)key, sd = (uint32_t)(key >> 32);
                if (sd < sad) { sad = sd; x = (int16_t)(idx & 0xffffu); y = (int16_t)(idx >> 16); }
            }
        }
        st->hme_sad[lvl][k] = sad * 2;
        x = (int16_t)(x + st->hme_cox[k]); x = (int16_t)(x * scale);
        y = (int16_t)(y + st->hme_coy[k]); y = (int16_t)(y * scale);
        st->hme_x[lvl][k] = x; st->hme_y[lvl][k] = y;
    }
}

/* pick the search centre from the last enabled level (run by ONE thread), Codec/EbMotionEstimation.c:4880-4980 */
SVT_DEV void me_hme_select(const me_ctx_t *c, int list) {
    const svt_me_params *p  = c->p;
    me_state_t          *st = c->st;
    const int            NW = p->number_hme_search_region_in_width, NH = p->number_hme_search_region_in_height;
    const int            lvl = p->enable_hme_level_2_flag ? 2 : p->enable_hme_level_1_flag ? 1 : 0;
    if (!p->enable_hme_level_0_flag && lvl == 0) return; /* no level ran: the previous result stays */
    int16_t  xc = st->hme_x[lvl][0], yc = st->hme_y[lvl][0];
    uint64_t sd = st->hme_sad[lvl][0];
    if (!(lvl == 0 && p->single_hme_quadrant)) {
        for (int k = 1; k < 4; k++) {
            if ((k & 1) >= NW || (k >> 1) >= NH) continue;
            if (st->hme_sad[lvl][k] < sd) { xc = st->hme_x[lvl][k]; yc = st->hme_y[lvl][k]; sd = st->hme_sad[lvl][k]; }
        }
        st->hme_rh = NH;
    }
    if (lvl == 2) {
        /* [quirk] the reference sorts with the index pair (q / NW, q % NW) applied to its [rw][rh] arrays (:4943-4975):
         * element q is region rw = q / NW, rh = q % NW, i.e. slot (q % NW) * 2 + q / NW */
        const int tot = NH * NW;
        if (p->same_ref_poc && list == 1 && tot > 1) {
            for (int q = 0; q < tot - 1; q++)
                for (int n = q + 1; n < tot; n++) {
                    const int kq = (q % NW) * 2 + q / NW, kn = (n % NW) * 2 + n / NW;
                    if (st->hme_sad[2][kq] > st->hme_sad[2][kn]) {
                        const int16_t  tx = st->hme_x[2][kq], ty = st->hme_y[2][kq];
                        const uint64_t td = st->hme_sad[2][kq];
                        st->hme_x[2][kq] = st->hme_x[2][kn]; st->hme_y[2][kq] = st->hme_y[2][kn]; st->hme_sad[2][kq] = st->hme_sad[2][kn];
                        st->hme_x[2][kn] = tx; st->hme_y[2][kn] = ty; st->hme_sad[2][kn] = td;
                    }
                }
            xc = st->hme_x[2][2]; yc = st->hme_y[2][2]; /* element [0][1] of the reference's arrays: rw = 0, rh = 1 */
        }
    }
    st->hme_xc = xc; st->hme_yc = yc;
}

#ifndef SVT_HOST_EMU /* device only: me_hme_lanes; the emulation runs me_hme_finish_level / me_hme_plan_level on one thread; pinned by tests/test_gpu_me.py::test_me_presets_vs_oracle */
/* The single-thread sections between the phases of an HME level -- results of level `fin` (me_hme_finish_level), plan of level `plan`
 * (me_hme_plan_level); either may be -1 -- spread over lanes 0..3 of wave 0: lane k owns region slot k = rh * 2 + rw.  The regions are
 * independent up to the packing of their windows into the scratch (prefix sums over the four lanes); when the level's windows do not fit
 * the scratch together (the 64x64-area presets' level 0) lane 0 plans the level with the sequential code.  The serial chain of LDS round
 * trips and reciprocal loads of one lane was 17 - 21 % of a workgroup's time at 1080p / 360p (SVT_HIP_ME_PROFILE); same results. */
SVT_DEV uint32_t me_magic_lane(int d) { return d <= 256 ? me_magics.v[d] : me_magic_of(d); }
SVT_DEV void me_hme_lanes(const me_ctx_t *c, int tid, int list, int fin, int plan, int16_t xsc, int16_t ysc, int first) {
    if (tid >= 4) return;
    const svt_me_params *p  = c->p;
    me_state_t          *st = c->st;
    const int            NW = p->number_hme_search_region_in_width, NH = p->number_hme_search_region_in_height;
    const int            k = tid, rw = k & 1, rh = k >> 1;
    const bool           valid = rw < NW && rh < NH;
    if (fin >= 0 && valid) {
        const int scale = 4 >> fin;
        uint64_t  sad = 0xffffff;
        int16_t   x = st->hme_x[fin][k], y = st->hme_y[fin][k];
        if (st->hme_cw[k] > 0) {
            const uint64_t key = st->hme_keys[k];
            if (key != ~0ull) {
                const uint32_t idx = (uint32_t)key, sd = (uint32_t)(key >> 32);
                if (sd < sad) { sad = sd; x = (int16_t)(idx & 0xffffu); y = (int16_t)(idx >> 16); }
            }
        }
        st->hme_sad[fin][k] = sad * 2;
        x = (int16_t)(x + st->hme_cox[k]); x = (int16_t)(x * scale);
        y = (int16_t)(y + st->hme_coy[k]); y = (int16_t)(y * scale);
        st->hme_x[fin][k] = x; st->hme_y[fin][k] = y;
    }
    if (plan < 0) return;
    me_hme_geom g;
    me_hme_geom_of(c, list, plan, &g);
    const int span = 2 * (g.bh - 1);
    if (first) { /* [quirk] centres are only initialised while the reference's row counter is below NH */
        const int rh_old = st->hme_rh;
        if (rh_old < NH && valid && rh >= rh_old) {
            st->hme_x[0][k] = (int16_t)(xsc >> 2); st->hme_y[0][k] = (int16_t)(ysc >> 2);
            st->hme_x[1][k] = (int16_t)(xsc >> 1); st->hme_y[1][k] = (int16_t)(ysc >> 1);
            st->hme_x[2][k] = xsc; st->hme_y[2][k] = ysc;
        }
    }
    { uint32_t *kw_ = (uint32_t *)&st->hme_keys[k]; kw_[0] = ~0u; kw_[1] = ~0u; }
    int16_t w = 0, h = 0, ox = 0, oy = 0;
    if (valid) {
        if (plan == 0) {
            w = rw ? c->L.hme_w0[1] : c->L.hme_w0[0]; /* (selects: a lane-dependent index would move the whole structure to scratch memory) */
            h = rh ? c->L.hme_h0[1] : c->L.hme_h0[0];
            int16_t ddx = (int16_t)(xsc >> 2), ddy = (int16_t)(ysc >> 2);
            if (rw > 0) ddx = (int16_t)(ddx + c->L.hme_w0[0]);
            if (rh > 0) ddy = (int16_t)(ddy + c->L.hme_h0[0]);
            ox = (int16_t)(-(int16_t)(c->L.hme_tw0 >> 1) + ddx);
            oy = (int16_t)(-(int16_t)(c->L.hme_th0 >> 1) + ddy);
        } else if (plan == 1) {
            w  = me_hme_round_w((int16_t)(rw ? p->hme_level1_search_area_in_width_array[1] : p->hme_level1_search_area_in_width_array[0]));
            h  = (int16_t)(rh ? p->hme_level1_search_area_in_height_array[1] : p->hme_level1_search_area_in_height_array[0]);
            ox = (int16_t)(-(w >> 1) + (int16_t)(st->hme_x[0][k] >> 1));
            oy = (int16_t)(-(h >> 1) + (int16_t)(st->hme_y[0][k] >> 1));
        } else {
            w  = me_hme_round_w((int16_t)(rw ? p->hme_level2_search_area_in_width_array[1] : p->hme_level2_search_area_in_width_array[0]));
            h  = (int16_t)(rh ? p->hme_level2_search_area_in_height_array[1] : p->hme_level2_search_area_in_height_array[0]);
            ox = (int16_t)(-(w >> 1) + st->hme_x[1][k]);
            oy = (int16_t)(-(h >> 1) + st->hme_y[1][k]);
        }
        me_clip_area(g.ox, &ox, &w, g.pad_w, g.ref_w);
        me_clip_area(g.oy, &oy, &h, g.pad_h, g.ref_h);
    }
    const bool ok = valid && w > 0 && h > 0;
    st->hme_cox[k] = valid ? ox : (int16_t)0; st->hme_coy[k] = valid ? oy : (int16_t)0; /* kept even when nothing is searched: the centre still moves by them */
    st->hme_cw[k] = ok ? w : (int16_t)0; st->hme_ch[k] = ok ? h : (int16_t)0;
    const int wbytes = w + g.bw + 3;
    int       ws     = ((wbytes + 3) & ~3) + 4;
    if (((ws >> 2) & 1) == 0) ws += 4;
    const int nd = (wbytes + 3) >> 2, ng = (g.bw & 3) == 0 ? (w + 3) >> 2 : w;
    const int my_bytes = ok ? ws * (h + span) : 0, my_tl = ok ? ME_HME_UNITS(nd) * (h + span) : 0, my_ts = ok ? ng * h : 0;
    int       bytes = 0, tl = 0, ts = 0, ne = 0, total = 0, n_all = 0;
    _Pragma("unroll") for (int j = 0; j < 4; j++) {
        const int bj = __shfl(my_bytes, j), tlj = __shfl(my_tl, j), tsj = __shfl(my_ts, j), okj = __shfl((int)ok, j);
        if (j < k) { bytes += bj; tl += tlj; ts += tsj; ne += okj; }
        total += bj; n_all += okj;
    }
    if (total <= c->hme_scratch_bytes) { /* one batch, one window per region */
        if (ok) {
            me_hme_win *wn = &st->hme_win[ne];
            wn->off = (uint32_t)bytes; wn->wstride = (uint16_t)ws; wn->nd = (uint8_t)nd; wn->rows = (uint16_t)(h + span); wn->sw = (uint16_t)w; wn->sh = (uint16_t)h;
            wn->gx = (int16_t)(g.ox + ox); wn->gy = (int16_t)(g.oy + oy); wn->slot = (uint8_t)k; wn->y0 = 0; wn->tl = (uint16_t)tl; wn->ts = (uint16_t)ts;
            wn->inv_nu = me_magic_lane(ME_HME_UNITS(nd)); wn->inv_ng = me_magic_lane(ng);
        }
        if (k == 0) { st->hme_rh = NH; st->hme_bstart[0] = 0; st->hme_bstart[1] = n_all; st->hme_nbatch = n_all > 0 ? 1 : 0; }
    } else if (k == 0) me_hme_plan_level(c, list, plan, xsc, ysc, first); /* bands: the sequential planner (it repeats the steps above) */
}
#endif

#endif
