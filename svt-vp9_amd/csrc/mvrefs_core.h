/*
 * mvrefs_core.h -- the rules of the MV-reference derivation, written once as plain inline functions that compile both for the device
 * (csrc/mvrefs.hip) and for the host (host/mvrefs_host.c), beside modeinfo_inter_core.h, whose inputs (svt_mi_inter_ext's ref_mv_row /
 * ref_mv_col / mode_context) they produce.
 *
 * What the reference derives per block of 8x8 or larger of a picture that is not intra-only, eb_vp9_find_mv_refs
 * (VPX/vp9_mvref_common.c:20-197 with vp9_mvref_common.h, called from prepare_fast_loop_candidates, Codec/EbModeDecision.c:638-672):
 * the two candidate MVs of a reference frame (NEARESTMV / NEARMV), how many of them it found, and the context of the inter mode.
 *
 * Why it is a function of the grid: the reference takes spatial candidates only; every one of the eight positions of a block's size
 * lies above or left of the block -- no more than 3 units above or left of its origin, never below its last row or right of its last
 * column --, so it belongs to a leaf that is final when the block is reached in coding order; and every 8x8 unit of a block
 * carries its block's values.  The inter mode alone is kept at a leaf's origin only (svt_mi_inter_ext), and blocks are aligned to their
 * size, so a candidate unit's own sb_type names the unit that holds its mode.
 *
 * The walk does not read the grids: it reads a window of 11 x 11 packed units that starts 3 units above and 3 left of the block's SB
 * (svt_mvr_pack builds an entry from the grids; the device stages the window in LDS, the host form in a local array), so both run the
 * same text.
 *
 *   svt_mvr_check    is the record of an 8x8 unit one this stage takes?
 *   svt_mvr_pack     the window entry of a unit: MV 0, MV 1 and a meta word
 *   svt_mvr_window_unit / _no_entry / _window_put, svt_mvr_view_of   building a window position by position, and a picture's view: the
 *                    text the device skeleton (mvrefs_stage.h) and the host forms share
 *   svt_mvr_derive   eb_vp9_find_mv_refs of one block and one reference frame: the two candidates, the return value
 *   svt_mvr_context  the mode context of a block (it does not depend on the reference frame)
 *   svt_mvr_unit     everything the stage writes for one unit
 *
 * The rule, restated (block side n units at (r, c), reference frame ref, `block` = -1: a candidate's MV is its block's, never a
 * sub-block's):
 *   pass 1   the eight positions of the block's size in order; one outside the picture (one tile) is passed over.  Positions 0 and 1
 *            add the counter class of the candidate's mode (any intra mode 9, NEARESTMV / NEARMV 0, ZEROMV 3, NEWMV 1).  A candidate
 *            offers mv[0] if ref_frame[0] == ref, else mv[1] if ref_frame[1] == ref.
 *   adding   the first MV goes to slot 0; a later one that differs from slot 0 in its 32 bits goes to slot 1 and ends the derivation
 *            ("done": return 2, both slots clamped)
 *   restrict (cm->use_prev_frame_mvs): not done after pass 1 -> return the count (0 or 1), clamp the found entry, the rest stays zero
 *   pass 2   (not restricted, not done, some position inside): the eight positions again, inter candidates only: mv[0] if
 *            ref_frame[0] != ref; then mv[1] if there is a second reference, ref_frame[1] != ref and mv[1] != mv[0] as 32-bit values;
 *            each with both components negated (wrapping in int16) when the sign biases of the candidate's reference and of ref differ
 *   clamp    col to [-(c * 64) - 128, (mi_cols - n - c) * 64 + 128], row likewise with r and mi_rows, in int
 */
#ifndef SVT_MVREFS_CORE_H
#define SVT_MVREFS_CORE_H

#include <stdint.h>
#include "modeinfo_core.h"

#define SVT_MVR_WIN 11                           /* the window's side in units: 3 above / left of the SB + its 8 */
#define SVT_MVR_WIN_WORDS (3 * SVT_MVR_WIN * SVT_MVR_WIN)

/* one picture's three grids of one mi_stride and the frame's parameters (svt_mvrefs_picture) */
typedef struct svt_mvr_view {
    const svt_lf_mode_info *mi;
    const svt_mc_mode_info *mc;
    const svt_mi_inter_ext *ext;
    uint8_t                 ref_mask, restrict_ref_mvs, sign_bias /* bit i: ref_frame_sign_bias[i] */, pad_[5];
} svt_mvr_view;

/* a window entry.  An MV is packed as the reference's int_mv: row in the low, col in the high 16 bits.  meta: bit 0 there (inside the
 * picture), 1 inter, 2 compound, 3-4 ref_frame[0], 5-6 ref_frame[1] (both 0 for an intra unit), 8-11 the counter class of the block's mode */
typedef struct svt_mvr_entry {
    uint32_t mv0, mv1, meta;
} svt_mvr_entry;
SVT_HD int svt_mvr_there(uint32_t m) { return (int)(m & 1); }
SVT_HD int svt_mvr_inter(uint32_t m) { return (int)(m >> 1 & 1); }
SVT_HD int svt_mvr_comp(uint32_t m) { return (int)(m >> 2 & 1); }
SVT_HD int svt_mvr_r0(uint32_t m) { return (int)(m >> 3 & 3); }
SVT_HD int svt_mvr_r1(uint32_t m) { return (int)(m >> 5 & 3); }
SVT_HD int svt_mvr_class(uint32_t m) { return (int)(m >> 8 & 15); }
SVT_HD uint32_t svt_mvr_mv(int row, int col) { return ((uint32_t)row & 0xFFFFu) | (uint32_t)col << 16; }
SVT_HD int svt_mvr_row(uint32_t mv) { return (int16_t)(mv & 0xFFFFu); }
SVT_HD int svt_mvr_col(uint32_t mv) { return (int16_t)(mv >> 16); }
/* level of a unit's block as the walks may trust it on any grid: a byte that is no block size counts as 8x8 */
SVT_HD int svt_mvr_level(int sb_type) { return sb_type > 12 ? 0 : svt_mi_level(sb_type); }

/* mv_ref_blocks of the square sizes (a constant of the format): position i of level l as (row + 3) | (col + 3) << 4 in byte i */
SVT_HD int svt_mvr_position(int l, int i) {
    const uint64_t t = l == 0 ? 0x1112211331222332ull : l == 1 ? 0x0003302224422332ull : l == 2 ? 0x0003302225522442ull : 0x9223322227722662ull;
    return (int)(t >> (8 * i) & 255);
}
/* counter_to_context over mode_2_counter's sums (constants of the format): of the counters 0 .. 8 only 0, 1, 2, 3, 4, 6 occur -> 2 3 4 1 3 . 0;
 * 9, 10, 12 (one intra neighbour) -> 5, 18 (two) -> 6 */
SVT_HD int svt_mvr_counter_context(int counter) { return counter >= 18 ? 6 : counter >= 9 ? 5 : (int)(0x990931432ull >> (4 * counter) & 15); }

/* 0: the unit (r, c) lies in a block this stage takes -- a square size, inside the picture and not claimed by a larger enclosing node;
 * reference frames up to 3; ref_frame, is_inter and the prediction grid's ref_list agreeing about inter and compound; no inter block
 * below 8x8; and, at an inter leaf's origin, the inter mode 10 .. 13.  (mode_context, ref_mv_*, tx_size and the frame's compound rules
 * belong to the stage behind this one and are not looked at.) */
SVT_HD int svt_mvr_check(const svt_mvr_view *v, const svt_tok_geom *g, int r, int c) {
    const int               idx = r * g->mi_stride + c;
    const svt_lf_mode_info *b = &v->mi[idx];
    const svt_mi_inter_ext *x = &v->ext[idx];
    const svt_mc_mode_info *m = &v->mc[idx];
    const int t = b->sb_type, inter = b->is_inter != 0, comp = x->ref_frame[1] > 0;
    if (t > 12 || t % 3) return 1;
    const int l = svt_mi_level(t), n = 1 << l;
    if ((r & ~(n - 1)) + n > g->mi_rows || (c & ~(n - 1)) + n > g->mi_cols) return 1;
    for (int L = l; L <= 3; L++) { /* (as svt_mi_check: no enclosing node's origin claims a larger block) */
        const int k = (1 << L) - 1, to = v->mi[(r & ~k) * g->mi_stride + (c & ~k)].sb_type;
        if (to > 12 || to % 3 || (L == l ? to != t : svt_mi_level(to) >= L)) return 1;
    }
    if (x->ref_frame[0] > 3 || x->ref_frame[1] > 3) return 1;
    if ((x->ref_frame[0] > 0) != inter || (m->ref_list[0] >= 0) != inter) return 1;
    if (!inter) return comp; /* (ref_list[0] < 0 says "not an inter block"; the prediction grid's other fields of such a unit mean nothing) */
    if (t == 0 || (m->ref_list[1] >= 0) != comp) return 1;
    if ((r | c) & (n - 1)) return 0;
    return x->mode < 10 || x->mode > 13;
}

/* the window entry of unit (r, c), which lies inside the picture.  Reads the unit's own three records and the mode at the origin of its
 * leaf; the MVs of an intra unit are not read.  In bounds on any grid. */
SVT_HD svt_mvr_entry svt_mvr_pack(const svt_mvr_view *v, const svt_tok_geom *g, int r, int c) {
    const int     idx = r * g->mi_stride + c, k = (1 << svt_mvr_level(v->mi[idx].sb_type)) - 1;
    svt_mvr_entry e;
    e.mv0 = e.mv1 = 0;
    e.meta = 1u | 9u << 8;
    if (v->mi[idx].is_inter) {
        const svt_mc_mode_info *m = &v->mc[idx];
        const int r0 = v->ext[idx].ref_frame[0] & 3, r1 = v->ext[idx].ref_frame[1] & 3, mode = v->ext[(r & ~k) * g->mi_stride + (c & ~k)].mode;
        e.mv0 = svt_mvr_mv(m->mv_row[0], m->mv_col[0]);
        e.mv1 = svt_mvr_mv(m->mv_row[1], m->mv_col[1]);
        e.meta = 1u | 2u | (uint32_t)(r1 > 0) << 2 | (uint32_t)r0 << 3 | (uint32_t)r1 << 5 | (uint32_t)(mode == 12 ? 3 : mode == 13 ? 1 : 0) << 8;
    }
    return e;
}
/* building the window of the SB whose first unit is (sb_r, sb_c), position i = 0 .. 120 at a time: the picture unit of the position and
 * whether it lies inside the picture; and the entry's three words at 3 * i -- a position outside the picture holds the zero entry (not
 * "there").  What packs an entry is the caller's: svt_mvr_pack here, svt_mdi_pack before the records exist (md_inter_core.h) */
SVT_HD int svt_mvr_window_unit(const svt_tok_geom *g, int sb_r, int sb_c, int i, int *r, int *c) {
    *r = sb_r - 3 + i / SVT_MVR_WIN; *c = sb_c - 3 + i % SVT_MVR_WIN;
    return *r >= 0 && *c >= 0 && *r < g->mi_rows && *c < g->mi_cols;
}
SVT_HD svt_mvr_entry svt_mvr_no_entry(void) {
    svt_mvr_entry e;
    e.mv0 = e.mv1 = e.meta = 0;
    return e;
}
SVT_HD void svt_mvr_window_put(uint32_t *win, int i, svt_mvr_entry e) { win[3 * i] = e.mv0; win[3 * i + 1] = e.mv1; win[3 * i + 2] = e.meta; }
/* the view of a picture from its descriptor's fields (svt_mvrefs_picture, svt_md_inter_picture) */
SVT_HD svt_mvr_view svt_mvr_view_of(const svt_lf_mode_info *mi, const svt_mc_mode_info *mc, const svt_mi_inter_ext *ext, int ref_mask, int restrict_ref_mvs,
                                    const uint8_t *ref_frame_sign_bias) {
    svt_mvr_view v = {0};
    v.mi = mi; v.mc = mc; v.ext = ext;
    v.ref_mask = (uint8_t)ref_mask; v.restrict_ref_mvs = restrict_ref_mvs != 0;
    for (int k = 0; k < 4; k++) v.sign_bias |= (uint8_t)((ref_frame_sign_bias[k] != 0) << k);
    return v;
}
SVT_HD svt_mvr_entry svt_mvr_window_at(const uint32_t *win, int wr, int wc) {
    const uint32_t *p = win + 3 * (wr * SVT_MVR_WIN + wc);
    svt_mvr_entry   e;
    e.mv0 = p[0]; e.mv1 = p[1]; e.meta = p[2];
    return e;
}

/* both components negated, wrapping in int16 (-32768 stays) */
SVT_HD uint32_t svt_mvr_negate(uint32_t mv) { return ((0u - (mv & 0xFFFFu)) & 0xFFFFu) | (0u - (mv >> 16)) << 16; }
SVT_HD int svt_mvr_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

/* the mode context of the block of level l at (r, c), window rows / columns wr, wc: the counter classes of positions 0 and 1 */
SVT_HD int svt_mvr_context(const uint32_t *win, int wr, int wc, int l) {
    int counter = 0;
    for (int i = 0; i < 2; i++) {
        const int      p = svt_mvr_position(l, i);
        const uint32_t m = win[3 * ((wr + (p & 15) - 3) * SVT_MVR_WIN + wc + (p >> 4) - 3) + 2];
        if (svt_mvr_there(m)) counter += svt_mvr_class(m);
    }
    return svt_mvr_counter_context(counter);
}

/* eb_vp9_find_mv_refs of the block of level l at picture unit (r, c) = window unit (wr, wc) (wr, wc >= 3) and reference frame ref
 * (1 .. 3): the two candidates, clamped as the reference clamps them (an entry it does not find is 0), and its return value */
SVT_HD int svt_mvr_derive(const svt_mvr_view *v, const svt_tok_geom *g, const uint32_t *win, int wr, int wc, int r, int c, int l, int ref, uint32_t *list0,
                          uint32_t *list1) {
    uint32_t l0 = 0, l1 = 0;
    int      count = 0, done = 0, any = 0;
    for (int i = 0; i < 8; i++) {
        const int           p = svt_mvr_position(l, i);
        const svt_mvr_entry e = svt_mvr_window_at(win, wr + (p & 15) - 3, wc + (p >> 4) - 3);
        if (done || !svt_mvr_there(e.meta)) continue;
        any = 1;
        const int first = svt_mvr_r0(e.meta) == ref;
        if (first || svt_mvr_r1(e.meta) == ref) {
            const uint32_t mv = first ? e.mv0 : e.mv1;
            if (!count) { l0 = mv; count = 1; }
            else if (mv != l0) { l1 = mv; done = 1; }
        }
    }
    if (!done && !v->restrict_ref_mvs && any) {
        const int bias = v->sign_bias >> ref & 1;
        for (int i = 0; i < 8; i++) {
            const int           p = svt_mvr_position(l, i);
            const svt_mvr_entry e = svt_mvr_window_at(win, wr + (p & 15) - 3, wc + (p >> 4) - 3);
            if (done || !svt_mvr_there(e.meta) || !svt_mvr_inter(e.meta)) continue;
            const int r0 = svt_mvr_r0(e.meta), r1 = svt_mvr_r1(e.meta);
            if (r0 != ref) {
                const uint32_t mv = (v->sign_bias >> r0 & 1) != bias ? svt_mvr_negate(e.mv0) : e.mv0;
                if (!count) { l0 = mv; count = 1; }
                else if (mv != l0) { l1 = mv; done = 1; }
            }
            if (!done && svt_mvr_comp(e.meta) && r1 != ref && e.mv1 != e.mv0) {
                const uint32_t mv = (v->sign_bias >> r1 & 1) != bias ? svt_mvr_negate(e.mv1) : e.mv1;
                if (!count) { l0 = mv; count = 1; }
                else if (mv != l0) { l1 = mv; done = 1; }
            }
        }
    }
    const int n = 1 << l, found = done ? 2 : count;
    const int col_lo = -(c * 64) - 128, col_hi = (g->mi_cols - n - c) * 64 + 128, row_lo = -(r * 64) - 128, row_hi = (g->mi_rows - n - r) * 64 + 128;
    if (found > 0) l0 = svt_mvr_mv(svt_mvr_clamp(svt_mvr_row(l0), row_lo, row_hi), svt_mvr_clamp(svt_mvr_col(l0), col_lo, col_hi));
    if (found > 1) l1 = svt_mvr_mv(svt_mvr_clamp(svt_mvr_row(l1), row_lo, row_hi), svt_mvr_clamp(svt_mvr_col(l1), col_lo, col_hi));
    *list0 = l0; *list1 = l1;
    return found;
}

/* what the stage writes for unit (r, c) of a well-formed grid, as the little-endian words of the records:
 *   ext[3]   svt_mi_inter_ext -- ref_frame of the unit's own record; at a leaf's origin its mode; at an inter leaf's origin slot 0 of
 *            the list of ref_frame[k] as ref_mv_row / ref_mv_col[k] and the mode context; everything else 0
 *   cand[8]  svt_mvref_cand -- at the origin of a leaf of 8x8 or larger (intra leaves as well) both candidates and the return value of
 *            every reference frame of ref_mask, and the mode context; count 0xFF for a frame not asked for; at any other unit all 0
 *            but the three counts, 0xFF
 *   inter_leaf, contradicts   an inter leaf's origin; and one whose coded MVs are not what its mode says: NEARESTMV with some
 *            mv[k] != slot 0 of ref_frame[k]'s list, NEARMV with some mv[k] != slot 1, ZEROMV with some mv[k] != 0 */
typedef struct svt_mvr_unit_out {
    uint32_t e0, e1, e2, k0, k1, k2, k3, k4, k5, k6, k7; /* (named words: an array indexed by the reference frame would live in scratch memory on the device) */
    int      inter_leaf, contradicts;
} svt_mvr_unit_out;
/* one reference frame of a leaf: derived if d_cand asks for it or the leaf uses it */
typedef struct svt_mvr_ref_out {
    uint32_t a, b;
    int      n;
} svt_mvr_ref_out;
SVT_HD svt_mvr_ref_out svt_mvr_ref(const svt_mvr_view *v, const svt_tok_geom *g, const uint32_t *win, int wr, int wc, int r, int c, int l, int ref, int wanted) {
    svt_mvr_ref_out o;
    o.a = o.b = 0;
    o.n = 0xFF;
    if (wanted) o.n = svt_mvr_derive(v, g, win, wr, wc, r, c, l, ref, &o.a, &o.b);
    return o;
}
SVT_HD svt_mvr_unit_out svt_mvr_unit(const svt_mvr_view *v, const svt_tok_geom *g, const uint32_t *win, int wr, int wc, int r, int c) {
    const int               idx = r * g->mi_stride + c;
    const svt_mi_inter_ext *x = &v->ext[idx];
    const int               t = v->mi[idx].sb_type, l = svt_mvr_level(t), inter = v->mi[idx].is_inter != 0;
    const int               origin = !((r | c) & ((1 << l) - 1));
    const int               f0 = x->ref_frame[0], f1 = x->ref_frame[1];
    svt_mvr_unit_out        o;
    o.e0 = o.e1 = 0;
    o.e2 = (uint32_t)f0 | (uint32_t)f1 << 8;
    o.k0 = o.k1 = o.k2 = o.k3 = o.k4 = o.k5 = o.k7 = 0;
    o.k6 = 0xFFFFFFu;
    o.inter_leaf = o.contradicts = 0;
    if (!origin) return o;
    const int mode = x->mode;
    o.e2 |= (uint32_t)mode << 16;
    if (t == 0) return o;
    const int ctx = svt_mvr_context(win, wr, wc, l), u0 = inter ? f0 : 0, u1 = inter ? f1 : 0;
    const int ask1 = v->ref_mask >> 1 & 1, ask2 = v->ref_mask >> 2 & 1, ask3 = v->ref_mask >> 3 & 1;
    const svt_mvr_ref_out q1 = svt_mvr_ref(v, g, win, wr, wc, r, c, l, 1, ask1 || u0 == 1 || u1 == 1);
    const svt_mvr_ref_out q2 = svt_mvr_ref(v, g, win, wr, wc, r, c, l, 2, ask2 || u0 == 2 || u1 == 2);
    const svt_mvr_ref_out q3 = svt_mvr_ref(v, g, win, wr, wc, r, c, l, 3, ask3 || u0 == 3 || u1 == 3);
    if (ask1) { o.k0 = (q1.a & 0xFFFFu) | q1.b << 16; o.k3 = q1.a >> 16 | (q1.b & 0xFFFF0000u); }
    if (ask2) { o.k1 = (q2.a & 0xFFFFu) | q2.b << 16; o.k4 = q2.a >> 16 | (q2.b & 0xFFFF0000u); }
    if (ask3) { o.k2 = (q3.a & 0xFFFFu) | q3.b << 16; o.k5 = q3.a >> 16 | (q3.b & 0xFFFF0000u); }
    o.k6 = (uint32_t)(ask1 ? q1.n : 0xFF) | (uint32_t)(ask2 ? q2.n : 0xFF) << 8 | (uint32_t)(ask3 ? q3.n : 0xFF) << 16 | (uint32_t)ctx << 24;
    if (!inter) return o;
    /* slot 0 and slot 1 of the lists of ref_frame[0] (a) and ref_frame[1] (b) */
    const uint32_t n0a = u0 == 1 ? q1.a : u0 == 2 ? q2.a : q3.a, n1a = u0 == 1 ? q1.b : u0 == 2 ? q2.b : q3.b;
    const uint32_t n0b = u1 == 0 ? 0 : u1 == 1 ? q1.a : u1 == 2 ? q2.a : q3.a, n1b = u1 == 0 ? 0 : u1 == 1 ? q1.b : u1 == 2 ? q2.b : q3.b;
    o.e0 = (n0a & 0xFFFFu) | n0b << 16;
    o.e1 = n0a >> 16 | (n0b & 0xFFFF0000u);
    o.e2 |= (uint32_t)ctx << 24;
    o.inter_leaf = 1;
    if (mode != 13) {
        const svt_mc_mode_info *m = &v->mc[idx];
        if (svt_mvr_mv(m->mv_row[0], m->mv_col[0]) != (mode == 10 ? n0a : mode == 11 ? n1a : 0)) o.contradicts = 1;
        if (u1 > 0 && svt_mvr_mv(m->mv_row[1], m->mv_col[1]) != (mode == 10 ? n0b : mode == 11 ? n1b : 0)) o.contradicts = 1;
    }
    return o;
}

#endif /* SVT_MVREFS_CORE_H */
