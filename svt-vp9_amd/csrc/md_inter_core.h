/*
 * md_inter_core.h -- the rules of inter mode labelling, written once as plain inline functions that compile both for the device
 * (csrc/md_inter.hip) and for the host (host/md_inter_host.c), on top of mvrefs_core.h (the candidates) and modeinfo_inter_core.h
 * (the frame's compound rules, use_mv_hp, the bound of a coded MV difference).
 *
 * What the stage decides: the svt_mi_inter_ext records the encode pass's grids lack -- ref_frame of every 8x8 unit and the inter mode
 * at every leaf origin --, such that svt_hip_mvrefs_* counts no leaf whose MVs contradict its mode.
 *
 * The rule:
 *   per unit        ref_frame[k] = ref_list[k] < 0 ? 0 : list_ref_frame[ref_list[k]]; an intra unit gets {0, 0}
 *   per inter leaf  (8x8 or larger) the two candidates of each of its reference frames by svt_mvr_derive, which reads the neighbours'
 *                   ref_frame and MVs only, never their modes -- so every leaf is labelled on its own, in parallel.  The leaf's MVs as
 *                   32-bit int_mv values against the clamped candidates, in this fixed order:
 *                     NEARESTMV  every reference's MV is its first candidate, and that candidate was found (count >= 1)
 *                     NEARMV     every reference's MV is its second candidate, and count == 2
 *                     ZEROMV     every MV is zero
 *                     NEWMV      otherwise
 *                   (The order does not look at inter_mode_probs[mode_context]: a choice by rate would make a leaf's label depend on its
 *                   neighbours' labels through the context counter.)
 *   then            mode_context and ref_mv_* exactly as svt_mvr_unit derives them from the labelled records
 *
 *   svt_mdi_ref_frame    ref_list[k] -> ref_frame[k]
 *   svt_mdi_pack         the window entry of a unit from the two grids alone (svt_mvr_pack takes ref_frame and the mode from records
 *                        that do not exist yet); the counter class is left 0: svt_mvr_derive does not read it
 *   svt_mdi_label        the mode of one inter leaf
 *   svt_mdi_label_unit   the third word of a unit's record: ref_frame[2], and at an inter leaf's origin the mode
 *   svt_mdi_check        what the labelled records must satisfy beyond svt_mvr_check: the frame's reference mode and compound pair
 *   svt_mdi_unfaithful   a NEWMV leaf whose MV pack_inter_mode_mvs / eb_vp9_encode_mv cannot code so that a decoder rebuilds it
 */
#ifndef SVT_MD_INTER_CORE_H
#define SVT_MD_INTER_CORE_H

#include <stdint.h>
#include "mvrefs_core.h"
#include "modeinfo_inter_core.h"

/* the frame's parameters beyond svt_mvr_view's (svt_md_inter_picture) */
typedef struct svt_mdi_frame {
    svt_mii_frame f;
    uint8_t       list_ref_frame[2];
    uint8_t       bad; /* list_ref_frame outside 1 .. 3: no grid is taken */
} svt_mdi_frame;
SVT_HD svt_mdi_frame svt_mdi_frame_of(const svt_md_inter_picture *p) {
    svt_mdi_frame m;
    m.f.reference_mode = p->reference_mode; m.f.allow_hp = p->allow_hp; m.f.comp_fixed_ref = p->comp_fixed_ref;
    m.f.comp_var_ref[0] = p->comp_var_ref[0]; m.f.comp_var_ref[1] = p->comp_var_ref[1];
    for (int i = 0; i < 4; i++) m.f.ref_frame_sign_bias[i] = p->ref_frame_sign_bias[i];
    m.list_ref_frame[0] = p->list_ref_frame[0]; m.list_ref_frame[1] = p->list_ref_frame[1];
    m.bad = p->list_ref_frame[0] < 1 || p->list_ref_frame[0] > 3 || p->list_ref_frame[1] < 1 || p->list_ref_frame[1] > 3;
    return m;
}

/* a list index the format does not know gives 0xFF, which svt_mvr_check refuses */
SVT_HD int svt_mdi_ref_frame(const svt_mdi_frame *m, int ref_list) { return ref_list < 0 ? 0 : ref_list > 1 ? 0xFF : m->list_ref_frame[ref_list]; }

/* the window entry of unit (r, c), which lies inside the picture: svt_mvr_pack with ref_frame taken from ref_list and no counter class.
 * In bounds on any grid. */
SVT_HD svt_mvr_entry svt_mdi_pack(const svt_mvr_view *v, const svt_mdi_frame *m, const svt_tok_geom *g, int r, int c) {
    const int     idx = r * g->mi_stride + c;
    svt_mvr_entry e;
    e.mv0 = e.mv1 = 0;
    e.meta = 1u;
    if (v->mi[idx].is_inter) {
        const svt_mc_mode_info *p = &v->mc[idx];
        const int r0 = svt_mdi_ref_frame(m, p->ref_list[0]) & 3, r1 = svt_mdi_ref_frame(m, p->ref_list[1]) & 3;
        e.mv0 = svt_mvr_mv(p->mv_row[0], p->mv_col[0]);
        e.mv1 = svt_mvr_mv(p->mv_row[1], p->mv_col[1]);
        e.meta = 1u | 2u | (uint32_t)(r1 > 0) << 2 | (uint32_t)r0 << 3 | (uint32_t)r1 << 5;
    }
    return e;
}

/* the mode of the inter leaf of level l at picture unit (r, c) = window unit (wr, wc) with reference frames f0 (1 .. 3) and f1 (0 .. 3) */
SVT_HD int svt_mdi_label(const svt_mvr_view *v, const svt_tok_geom *g, const uint32_t *win, int wr, int wc, int r, int c, int l, int f0, int f1) {
    const svt_mc_mode_info *p = &v->mc[r * g->mi_stride + c];
    const uint32_t mv0 = svt_mvr_mv(p->mv_row[0], p->mv_col[0]), mv1 = f1 ? svt_mvr_mv(p->mv_row[1], p->mv_col[1]) : 0;
    uint32_t a0, b0, a1 = 0, b1 = 0;
    const int n0 = svt_mvr_derive(v, g, win, wr, wc, r, c, l, f0, &a0, &b0);
    int       n1 = 2; /* (a single leaf: the second reference agrees with everything) */
    if (f1) n1 = svt_mvr_derive(v, g, win, wr, wc, r, c, l, f1, &a1, &b1);
    if (n0 >= 1 && n1 >= 1 && mv0 == a0 && mv1 == a1) return 10;
    if (n0 == 2 && n1 == 2 && mv0 == b0 && mv1 == b1) return 11;
    if (mv0 == 0 && mv1 == 0) return 12;
    return 13;
}

/* ref_frame[0] | ref_frame[1] << 8 | mode << 16 of unit (r, c) inside the picture, on any grid: the mode (else 0) at the origin of an inter
 * leaf of 8x8 or larger whose reference frames are ones the format knows -- any other grid is refused by the checks that follow */
SVT_HD uint32_t svt_mdi_label_unit(const svt_mvr_view *v, const svt_mdi_frame *m, const svt_tok_geom *g, const uint32_t *win, int wr, int wc, int r, int c) {
    const int idx = r * g->mi_stride + c, t = v->mi[idx].sb_type, l = svt_mvr_level(t);
    if (!v->mi[idx].is_inter) return 0;
    const int      f0 = svt_mdi_ref_frame(m, v->mc[idx].ref_list[0]), f1 = svt_mdi_ref_frame(m, v->mc[idx].ref_list[1]);
    const uint32_t w = (uint32_t)f0 | (uint32_t)f1 << 8;
    if (((r | c) & ((1 << l) - 1)) || t == 0 || t > 12 || f0 < 1 || f0 > 3 || f1 > 3) return w;
    return w | (uint32_t)svt_mdi_label(v, g, win, wr, wc, r, c, l, f0, f1) << 16;
}

/* 0: the labelled record of unit (r, c), which passed svt_mvr_check, fits the frame -- a compound block only where the reference mode
 * allows one, a single one only where it allows that, and a compound block's references are comp_fixed_ref plus one of comp_var_ref in
 * the order the sign bias gives (the condition of svt_mii_check) */
SVT_HD int svt_mdi_check(const svt_mvr_view *v, const svt_mdi_frame *m, const svt_tok_geom *g, int r, int c) {
    const int               idx = r * g->mi_stride + c;
    const svt_mi_inter_ext *x = &v->ext[idx];
    if (!v->mi[idx].is_inter) return 0;
    const int comp = x->ref_frame[1] > 0;
    if (comp ? m->f.reference_mode == SVT_MODES_SINGLE_REFERENCE : m->f.reference_mode == SVT_MODES_COMPOUND_REFERENCE) return 1;
    if (comp) {
        const int fix_idx = m->f.ref_frame_sign_bias[m->f.comp_fixed_ref & 3] != 0, var = x->ref_frame[!fix_idx];
        if (x->ref_frame[fix_idx] != m->f.comp_fixed_ref || (var != m->f.comp_var_ref[0] && var != m->f.comp_var_ref[1])) return 1;
    }
    return 0;
}

/* eb_vp9_encode_mv (VPX/vp9_encodemv.c) of mv against ref_mv: a difference beyond +-SVT_MII_MV_DIFF_MAX has no class; and where the
 * high-precision bit is not coded -- !(allow_hp && use_mv_hp(ref_mv)) -- a decoder takes it as set, so an odd difference comes back
 * one step longer */
SVT_HD int svt_mdi_unfaithful(int row, int col, int ref_row, int ref_col, int allow_hp) {
    const int dr = row - ref_row, dc = col - ref_col;
    if (svt_mii_abs(dr) > SVT_MII_MV_DIFF_MAX || svt_mii_abs(dc) > SVT_MII_MV_DIFF_MAX) return 1;
    return !(allow_hp && svt_mii_use_mv_hp(ref_row, ref_col)) && ((dr | dc) & 1);
}
/* the two counts of a finished record (svt_mvr_unit_out): a NEWMV leaf, and one that some reference's MV makes unfaithful */
SVT_HD void svt_mdi_count(const svt_mvr_view *v, const svt_mdi_frame *m, const svt_tok_geom *g, int r, int c, const svt_mvr_unit_out *o, int *newmv, int *unfaithful) {
    *newmv = *unfaithful = 0;
    if (!o->inter_leaf || (o->e2 >> 16 & 255) != 13) return;
    const svt_mc_mode_info *p = &v->mc[r * g->mi_stride + c];
    *newmv = 1;
    *unfaithful = svt_mdi_unfaithful(p->mv_row[0], p->mv_col[0], (int16_t)(o->e0 & 0xFFFFu), (int16_t)(o->e1 & 0xFFFFu), m->f.allow_hp);
    if (o->e2 >> 8 & 255) *unfaithful |= svt_mdi_unfaithful(p->mv_row[1], p->mv_col[1], (int16_t)(o->e0 >> 16), (int16_t)(o->e1 >> 16), m->f.allow_hp);
}

#endif /* SVT_MD_INTER_CORE_H */
