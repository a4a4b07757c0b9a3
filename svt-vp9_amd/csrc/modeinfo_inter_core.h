/*
 * modeinfo_inter_core.h -- the rules of the mode-info syntax of inter pictures, written once as plain inline functions that compile both
 * for the device (csrc/modeinfo_inter.hip) and for the host (host/modeinfo_inter_host.c), beside modeinfo_core.h, whose partition walk,
 * intra mode tree and token runs it shares.
 *
 * What the reference codes per block in front of its tokens in a picture that is not intra-only (Codec/EbEntropyCodingProcess.c:60-449
 * over write_partition, VPX/vp9_bitstream.c:399-417, and pack_inter_mode_mvs, :206-321), as raw bool records for the bool coder's
 * kind-1 segments.  The argument at the head of modeinfo_core.h carries over unchanged: every context of this syntax
 * (vp9_get_skip_context, get_intra_inter_context, eb_vp9_get_reference_mode_context, eb_vp9_get_pred_context_single_ref_p1 / _p2,
 * eb_vp9_get_pred_context_comp_ref_p; VPX/vp9_pred_common.[ch]) reads xd->above_mi and xd->left_mi only, which are the leaves that
 * cover (r - 1, c) and (r, c - 1) of the leaf's origin (NULL in picture row 0 / column 0: one tile), and of them only the skip flag,
 * ref_frame[0] and ref_frame[1] -- every unit of a block carries its block's values.  So every context is a function of the grid.
 *
 *   svt_mii_check        is the record of an 8x8 unit one this syntax takes?
 *   svt_mii_unit_bools   the bools that start at an 8x8 unit: the partition symbols of every node whose origin it is, then -- the unit
 *                        is a leaf's origin -- skip, is_inter, and the intra modes or reference frames, inter mode and MV differences
 *
 * The bound on the bools that start at one unit, from the trees (VPX/vp9_entropymode.c, VPX/vp9_entropymv.c):
 *   partition        the nodes of 64, 32 and 16 above a leaf's origin are SPLIT = 1 1 1, 3 bools each; the 8x8 node is SPLIT (3 bools)
 *                    only over four 4x4 blocks, which are intra -- over an 8x8 leaf it is NONE, 1 bool: 12 intra, 10 inter
 *   skip, is_inter                                                                                                  2
 *   an intra leaf    4 luma modes + the chroma mode, 7 bools each (D153, D207): 35                                  -> 12 + 2 + 35 = 49
 *   an inter leaf    references: the compound flag (REFERENCE_MODE_SELECT) + 1 bool of a compound block, or + 2 of a single one
 *                    inter mode: eb_vp9_inter_mode_tree, 3 bools (NEARMV, NEWMV)
 *                    one MV difference: the joint, 3 bools (eb_vp9_mv_joint_tree), and per component the sign 1, the class 7 --
 *                    eb_vp9_mv_class_tree has 10 probabilities, but its longest paths, those of classes 7 .. 10, visit 7 nodes --,
 *                    the integer bits 10 (class 10; class c > 0 has c, class 0 has 1), the fraction 3 (eb_vp9_mv_fp_tree), the
 *                    high-precision bit 1: 22 a component, 3 + 2 * 22 = 47 a difference
 *                    a single-reference NEWMV leaf: 10 + 2 + 3 + 3 + 47 = 65; a compound one: 10 + 2 + 2 + 3 + 2 * 47 = 111
 * The compound NEWMV 8x8 leaf at the origin of an SB is the maximum: SVT_MII_UNIT_BOOLS = 111.  (A class-10 component with the
 * high-precision bit needs a reference MV below 64 and a difference above 8192 in magnitude: both fit an int16 MV.)
 */
#ifndef SVT_MODEINFO_INTER_CORE_H
#define SVT_MODEINFO_INTER_CORE_H

#include <stdint.h>
#include "modeinfo_core.h"

#define SVT_MII_MV_COMP_BOOLS (1 + 7 + 10 + 3 + 1)
#define SVT_MII_MV_BOOLS (3 + 2 * SVT_MII_MV_COMP_BOOLS)
#define SVT_MII_UNIT_BOOLS (3 * 3 + 1 + 2 + 2 + 3 + 2 * SVT_MII_MV_BOOLS)
#define SVT_MII_MV_DIFF_MAX 16383 /* MV_UPP: (1 << MV_IN_USE_BITS) - 1 (VPX/vp9_entropymv.h) */

/* the frame's parameters (svt_modes_inter_picture) */
typedef struct svt_mii_frame {
    uint8_t reference_mode, allow_hp, comp_fixed_ref, comp_var_ref[2], ref_frame_sign_bias[4];
} svt_mii_frame;
SVT_HD svt_mii_frame svt_mii_frame_of(const svt_modes_inter_picture *p) {
    svt_mii_frame f;
    f.reference_mode = p->reference_mode; f.allow_hp = p->allow_hp; f.comp_fixed_ref = p->comp_fixed_ref;
    f.comp_var_ref[0] = p->comp_var_ref[0]; f.comp_var_ref[1] = p->comp_var_ref[1];
    for (int i = 0; i < 4; i++) f.ref_frame_sign_bias[i] = p->ref_frame_sign_bias[i];
    return f;
}
/* the parameters the entry points take: a reference mode 0 .. 2 and, where compound blocks may occur, references 1 .. 3 */
SVT_HD int svt_mii_bad_frame(const svt_mii_frame *f) {
    if (f->reference_mode > SVT_MODES_REFERENCE_SELECT) return 1;
    if (f->reference_mode == SVT_MODES_SINGLE_REFERENCE) return 0;
    return f->comp_fixed_ref < 1 || f->comp_fixed_ref > 3 || f->comp_var_ref[0] < 1 || f->comp_var_ref[0] > 3 || f->comp_var_ref[1] < 1 || f->comp_var_ref[1] > 3;
}
/* one picture's three grids of one mi_stride */
typedef struct svt_mii_view {
    const svt_lf_mode_info *mi;
    const svt_mc_mode_info *mc;
    const svt_mi_inter_ext *ext;
    svt_mii_frame           f;
} svt_mii_view;

/* a neighbour as the contexts see it, packed into one int so that the contexts select between two of them by value (pointers to them
 * would put them into scratch memory on the device): bit 0 there (inside the picture), 1 intra, 2 compound, 3-4 ref_frame[0],
 * 5-6 ref_frame[1], 7 skip */
#define SVT_MII_NB_NONE 2
SVT_HD int svt_mii_neighbour(const svt_mii_view *v, int there, int idx) {
    if (!there) return SVT_MII_NB_NONE;
    const int r0 = v->ext[idx].ref_frame[0] & 3, r1 = v->ext[idx].ref_frame[1] & 3;
    return 1 | (r0 == 0) << 1 | (r1 > 0) << 2 | r0 << 3 | r1 << 5 | (v->mi[idx].skip != 0) << 7;
}
SVT_HD int svt_nb_there(int n) { return n & 1; }
SVT_HD int svt_nb_intra(int n) { return (n >> 1) & 1; }
SVT_HD int svt_nb_comp(int n) { return (n >> 2) & 1; }
SVT_HD int svt_nb_r0(int n) { return (n >> 3) & 3; }
SVT_HD int svt_nb_r1(int n) { return (n >> 5) & 3; }
SVT_HD int svt_nb_skip(int n) { return (n >> 7) & 1; }
/* does the block use reference `ref` (in either place of a compound block)? */
SVT_HD int svt_nb_uses(int n, int ref) { return svt_nb_r0(n) == ref || (svt_nb_comp(n) && svt_nb_r1(n) == ref); }

/* get_intra_inter_context: both there -> 3 both intra, 1 one intra, 0 none; one there -> 2 if it is intra; none -> 0 */
SVT_HD int svt_mii_ctx_intra_inter(int a, int l) {
    if (svt_nb_there(a) && svt_nb_there(l)) return svt_nb_intra(a) && svt_nb_intra(l) ? 3 : (svt_nb_intra(a) || svt_nb_intra(l));
    if (svt_nb_there(a) || svt_nb_there(l)) return 2 * svt_nb_intra(svt_nb_there(a) ? a : l);
    return 0;
}
/* eb_vp9_get_reference_mode_context: the context of the compound flag */
SVT_HD int svt_mii_ctx_comp_inter(int a, int l, int fixed) {
    if (svt_nb_there(a) && svt_nb_there(l)) {
        if (svt_nb_comp(a) && svt_nb_comp(l)) return 4;
        if (!svt_nb_comp(a) && !svt_nb_comp(l)) return (svt_nb_r0(a) == fixed) ^ (svt_nb_r0(l) == fixed);
        const int s = svt_nb_comp(a) ? l : a; /* the single (or intra) one of the two */
        return 2 + (svt_nb_r0(s) == fixed || svt_nb_intra(s));
    }
    if (svt_nb_there(a) || svt_nb_there(l)) {
        const int e = svt_nb_there(a) ? a : l;
        return svt_nb_comp(e) ? 3 : svt_nb_r0(e) == fixed;
    }
    return 1;
}
/* eb_vp9_get_pred_context_single_ref_p1: the context of "not LAST" */
SVT_HD int svt_mii_ctx_single_p1(int a, int l) {
    const int both = svt_nb_there(a) && svt_nb_there(l);
    if (!svt_nb_there(a) && !svt_nb_there(l)) return 2;
    if (both && svt_nb_intra(a) && svt_nb_intra(l)) return 2;
    if (!both || svt_nb_intra(a) || svt_nb_intra(l)) { /* one neighbour counts: the only one there, or the inter one of the two */
        const int e = !both ? (svt_nb_there(a) ? a : l) : (svt_nb_intra(a) ? l : a);
        if (svt_nb_intra(e)) return 2;
        return svt_nb_comp(e) ? 1 + svt_nb_uses(e, 1) : 4 * (svt_nb_r0(e) == 1);
    }
    if (svt_nb_comp(a) && svt_nb_comp(l)) return 1 + (svt_nb_uses(a, 1) || svt_nb_uses(l, 1));
    if (svt_nb_comp(a) || svt_nb_comp(l)) {
        const int s = svt_nb_comp(a) ? l : a, k = svt_nb_comp(a) ? a : l;
        return (svt_nb_r0(s) == 1 ? 3 : 0) + svt_nb_uses(k, 1);
    }
    return 2 * (svt_nb_r0(a) == 1) + 2 * (svt_nb_r0(l) == 1);
}
/* eb_vp9_get_pred_context_single_ref_p2: the context of "not GOLDEN" */
SVT_HD int svt_mii_ctx_single_p2(int a, int l) {
    const int both = svt_nb_there(a) && svt_nb_there(l);
    if (!svt_nb_there(a) && !svt_nb_there(l)) return 2;
    if (both && svt_nb_intra(a) && svt_nb_intra(l)) return 2;
    if (!both) {
        const int e = svt_nb_there(a) ? a : l;
        if (svt_nb_intra(e) || (svt_nb_r0(e) == 1 && !svt_nb_comp(e))) return 2;
        return svt_nb_comp(e) ? 3 * svt_nb_uses(e, 2) : 4 * (svt_nb_r0(e) == 2);
    }
    if (svt_nb_intra(a) || svt_nb_intra(l)) {
        const int e = svt_nb_intra(a) ? l : a;
        if (svt_nb_comp(e)) return 1 + 2 * svt_nb_uses(e, 2);
        return svt_nb_r0(e) == 1 ? 3 : 4 * (svt_nb_r0(e) == 2);
    }
    if (svt_nb_comp(a) && svt_nb_comp(l))
        return svt_nb_r0(a) == svt_nb_r0(l) && svt_nb_r1(a) == svt_nb_r1(l) ? 3 * (svt_nb_uses(a, 2) || svt_nb_uses(l, 2)) : 2;
    if (svt_nb_comp(a) || svt_nb_comp(l)) {
        const int s = svt_nb_comp(a) ? l : a, k = svt_nb_comp(a) ? a : l, g = svt_nb_uses(k, 2);
        return svt_nb_r0(s) == 2 ? 3 + g : svt_nb_r0(s) == 3 ? g : 1 + 2 * g;
    }
    if (svt_nb_r0(a) == 1 && svt_nb_r0(l) == 1) return 3;
    if (svt_nb_r0(a) == 1 || svt_nb_r0(l) == 1) return 4 * ((svt_nb_r0(a) == 1 ? svt_nb_r0(l) : svt_nb_r0(a)) == 2);
    return 2 * (svt_nb_r0(a) == 2) + 2 * (svt_nb_r0(l) == 2);
}
/* eb_vp9_get_pred_context_comp_ref_p: the context of the compound block's variable reference */
SVT_HD int svt_mii_ctx_comp_ref(int a, int l, const svt_mii_frame *f) {
    const int fixed = f->comp_fixed_ref, v0 = f->comp_var_ref[0], v1 = f->comp_var_ref[1], var_idx = !f->ref_frame_sign_bias[fixed & 3];
    const int both = svt_nb_there(a) && svt_nb_there(l);
    /* the reference a neighbour varies: its only one, or a compound block's variable one */
    const int va = svt_nb_comp(a) && var_idx ? svt_nb_r1(a) : svt_nb_r0(a), vl = svt_nb_comp(l) && var_idx ? svt_nb_r1(l) : svt_nb_r0(l);
    if (!svt_nb_there(a) && !svt_nb_there(l)) return 2;
    if (!both) {
        const int e = svt_nb_there(a) ? a : l, ve = svt_nb_there(a) ? va : vl;
        if (svt_nb_intra(e)) return 2;
        return svt_nb_comp(e) ? 4 * (ve != v1) : 3 * (ve != v1);
    }
    if (svt_nb_intra(a) && svt_nb_intra(l)) return 2;
    if (svt_nb_intra(a) || svt_nb_intra(l)) return 1 + 2 * ((svt_nb_intra(a) ? vl : va) != v1);
    if (va == vl && va == v1) return 0;
    if (!svt_nb_comp(a) && !svt_nb_comp(l)) return (va == fixed && vl == v0) || (vl == fixed && va == v0) ? 4 : va == vl ? 3 : 1;
    if (svt_nb_comp(a) && svt_nb_comp(l)) return va == vl ? 4 : 2;
    {
        const int vc = svt_nb_comp(a) ? va : vl, vs = svt_nb_comp(a) ? vl : va; /* the compound one's, the single one's */
        return vc == v1 && vs != v1 ? 1 : vs == v1 && vc != v1 ? 2 : 4;
    }
}

/* The four-leaf tree 0 | (1 | (2 | 3)) that eb_vp9_mv_joint_tree, eb_vp9_mv_fp_tree and eb_vp9_inter_mode_tree (leaves ZEROMV, NEARESTMV,
 * NEARMV, NEWMV) share: leaf v is v ones and, below 3, a zero, under probs[0 ..].  out may be NULL. */
SVT_HD int svt_mii_tree4(int v, const uint8_t *probs, uint16_t *out) {
    const int len = v < 3 ? v + 1 : 3;
    if (out)
        for (int k = 0; k < len; k++) out[k] = SVT_BOOL_RECORD(k < v, probs[k]);
    return len;
}
/* eb_vp9_mv_class_tree: 0 | (1 | ((2 | 3) | ((4 | 5) | (6 | ((7 | 8) | (9 | 10)))))), nodes numbered as its probabilities are.
 * A class's path: its length, its bits from the top, and the node of step k */
SVT_HD int svt_mii_class_len(int c) { return (int)((0x77775554421ull >> (4 * c)) & 15); }
SVT_HD int svt_mii_class_path(int c) { return (int)((c < 8 ? 0x7C1E1D1C0D0C0200ull >> (8 * c) : 0x7F7E7Dull >> (8 * (c - 8))) & 255); }
SVT_HD int svt_mii_class_node(int c, int k) { return k < 3 ? k : k == 3 ? (c < 4 ? 3 : 4) : k == 4 ? (c < 6 ? 5 : 6) : k == 5 ? 7 : (c < 9 ? 8 : 9); }
/* eb_vp9_get_mv_class: class of z = |component| - 1 (class 0: 0 .. 15, class c: 8 << c .. (16 << c) - 1, class 10 open-ended) */
SVT_HD int svt_mii_mv_class(int z) {
    int c = 0;
    for (int k = z >> 4; k && c < 10; k >>= 1) c++;
    return c;
}
/* encode_mv_component: sign, class, integer bits (class 0: one bool; class c: c bools, LSB first), fraction, high-precision bit */
SVT_HD int svt_mii_mv_comp_bools(int comp, int usehp, const svt_modes_mv_comp *p, uint16_t *out) {
    const int sign = comp < 0, z = (sign ? -comp : comp) - 1, c = svt_mii_mv_class(z), o = z - (c ? 8 << c : 0), d = o >> 3, fr = (o >> 1) & 3;
    const int clen = svt_mii_class_len(c);
    int       n = 0;
    if (out) {
        const int path = svt_mii_class_path(c);
        out[n] = SVT_BOOL_RECORD(sign, p->sign);
        for (int k = 0; k < clen; k++) out[n + 1 + k] = SVT_BOOL_RECORD((path >> (clen - 1 - k)) & 1, p->classes[svt_mii_class_node(c, k)]);
    }
    n += 1 + clen;
    if (c == 0) {
        if (out) out[n] = SVT_BOOL_RECORD(d, p->class0[0]);
        n++;
    } else {
        if (out)
            for (int i = 0; i < c; i++) out[n + i] = SVT_BOOL_RECORD((d >> i) & 1, p->bits[i]);
        n += c;
    }
    n += svt_mii_tree4(fr, out ? (c == 0 ? p->class0_fp[d] : p->fp) : (const uint8_t *)0, out ? out + n : (uint16_t *)0);
    if (usehp) {
        if (out) out[n] = SVT_BOOL_RECORD(o & 1, c == 0 ? p->class0_hp : p->hp);
        n++;
    }
    return n;
}
/* eb_vp9_encode_mv: the joint, then the vertical and the horizontal component where they are not zero.  usehp = allow_hp && use_mv_hp(ref) */
SVT_HD int svt_mii_mv_bools(int drow, int dcol, int usehp, const svt_modes_inter_tables *t, uint16_t *out) {
    int n = svt_mii_tree4(2 * (drow != 0) + (dcol != 0), out ? t->mv_joints : (const uint8_t *)0, out);
    if (drow) n += svt_mii_mv_comp_bools(drow, usehp, out ? &t->mv_comps[0] : (const svt_modes_mv_comp *)0, out ? out + n : (uint16_t *)0);
    if (dcol) n += svt_mii_mv_comp_bools(dcol, usehp, out ? &t->mv_comps[1] : (const svt_modes_mv_comp *)0, out ? out + n : (uint16_t *)0);
    return n;
}
SVT_HD int svt_mii_abs(int v) { return v < 0 ? -v : v; }
/* use_mv_hp (VPX/vp9_entropymv.h): the high-precision bit of a difference is coded only against a reference MV below 8 samples */
SVT_HD int svt_mii_use_mv_hp(int ref_row, int ref_col) { return svt_mii_abs(ref_row) < 64 && svt_mii_abs(ref_col) < 64; }

/* 0: the unit (r, c) lies in a block this syntax takes -- what svt_mi_check asks of a key frame's unit but for is_inter, and:
 * ref_frame, is_inter and the prediction grid's ref_list agree about inter and compound; an inter block is 8x8 or larger; a compound
 * block fits the frame's reference mode and its fixed / variable references; and, at a leaf's origin, the inter mode is 10 .. 13, the
 * mode context at most 6 and a NEWMV block's MV differences are within +-SVT_MII_MV_DIFF_MAX */
SVT_HD int svt_mii_check(const svt_mii_view *v, const svt_tok_geom *g, int r, int c) {
    const int               idx = r * g->mi_stride + c;
    const svt_lf_mode_info *b = &v->mi[idx];
    const svt_mi_inter_ext *x = &v->ext[idx];
    const svt_mc_mode_info *m = &v->mc[idx];
    const int t = b->sb_type, inter = b->is_inter != 0, comp = x->ref_frame[1] > 0;
    if (t > 12 || t % 3) return 1;
    const int l = svt_mi_level(t), n = 1 << l;
    if ((r & ~(n - 1)) + n > g->mi_rows || (c & ~(n - 1)) + n > g->mi_cols) return 1;
    if (b->tx_size != (t == 0 ? 0 : l < 2 ? l + 1 : 3)) return 1;
    for (int L = l; L <= 3; L++) { /* (as svt_mi_check: no enclosing node's origin claims a larger block) */
        const int k = (1 << L) - 1, to = v->mi[(r & ~k) * g->mi_stride + (c & ~k)].sb_type;
        if (to > 12 || to % 3 || (L == l ? to != t : svt_mi_level(to) >= L)) return 1;
    }
    if (x->ref_frame[0] > 3 || x->ref_frame[1] > 3) return 1;
    if ((x->ref_frame[0] > 0) != inter || (m->ref_list[0] >= 0) != inter) return 1;
    if (!inter) { /* (ref_list[0] < 0 says "not an inter block"; the prediction grid's other fields of such a unit mean nothing) */
        if (comp || b->pad_[2] > 9) return 1;
        for (int k = 0; k < (t ? 1 : 4); k++)
            if (svt_mi_y_mode(b, k) > 9) return 1;
        return 0;
    }
    if (t == 0 || (m->ref_list[1] >= 0) != comp) return 1;
    if (comp ? v->f.reference_mode == SVT_MODES_SINGLE_REFERENCE : v->f.reference_mode == SVT_MODES_COMPOUND_REFERENCE) return 1;
    if (comp) {
        const int fix_idx = v->f.ref_frame_sign_bias[v->f.comp_fixed_ref & 3] != 0, var = x->ref_frame[!fix_idx];
        if (x->ref_frame[fix_idx] != v->f.comp_fixed_ref || (var != v->f.comp_var_ref[0] && var != v->f.comp_var_ref[1])) return 1;
    }
    if ((r | c) & (n - 1)) return 0;
    if (x->mode < 10 || x->mode > 13 || x->mode_context > 6) return 1;
    if (x->mode == 13)
        for (int k = 0; k <= comp; k++)
            if (svt_mii_abs(m->mv_row[k] - x->ref_mv_row[k]) > SVT_MII_MV_DIFF_MAX || svt_mii_abs(m->mv_col[k] - x->ref_mv_col[k]) > SVT_MII_MV_DIFF_MAX) return 1;
    return 0;
}

/* The bools that start at unit (r, c) of a well-formed grid, in coding order; 0 when the unit is no leaf's origin.  out (and t) may be
 * NULL: the count alone, which needs neither probabilities nor neighbours -- it follows from the unit's own records, the picture edge,
 * the reference mode and the MV differences (joint, class, fraction, and whether the high-precision bit is coded).  At most
 * SVT_MII_UNIT_BOOLS. */
SVT_HD int svt_mii_unit_bools(const svt_mii_view *v, const svt_tok_geom *g, int r, int c, const svt_modes_inter_tables *t, uint16_t *out) {
    const int               idx = r * g->mi_stride + c;
    const svt_lf_mode_info *b = &v->mi[idx];
    const int               ty = b->sb_type, l = svt_mi_level(ty);
    if ((r | c) & ((1 << l) - 1)) return 0;
    int n = 0;
    /* write_partition at every node whose origin this is, as in svt_mi_unit_bools, under the frame's probabilities */
    const int sa = out && r ? svt_mi_seg_context(v->mi[idx - g->mi_stride].sb_type) : 0, sl = out && c ? svt_mi_seg_context(v->mi[idx - 1].sb_type) : 0;
    for (int L = 3; L >= l; L--) {
        if ((r | c) & ((1 << L) - 1)) continue;
        const int hbs = (1 << L) >> 1, has_rows = r + hbs < g->mi_rows, has_cols = c + hbs < g->mi_cols, split = L > l || ty == 0;
        const uint8_t *p = out ? t->partition_prob[4 * L + 2 * ((sl >> L) & 1) + ((sa >> L) & 1)] : (const uint8_t *)0;
        if (has_rows && has_cols) {
            if (out) out[n] = SVT_BOOL_RECORD(split, p[0]);
            n++;
            if (split) {
                if (out) { out[n] = SVT_BOOL_RECORD(1, p[1]); out[n + 1] = SVT_BOOL_RECORD(1, p[2]); }
                n += 2;
            }
        } else if (has_rows || has_cols) {
            if (out) out[n] = SVT_BOOL_RECORD(1, p[has_cols ? 1 : 2]);
            n++;
        }
    }
    /* pack_inter_mode_mvs: skip, is_inter */
    const int inter = b->is_inter != 0;
    int a = SVT_MII_NB_NONE, lf = SVT_MII_NB_NONE;
    if (out) {
        a = svt_mii_neighbour(v, r > 0, idx - g->mi_stride);
        lf = svt_mii_neighbour(v, c > 0, idx - 1);
        out[n] = SVT_BOOL_RECORD(b->skip ? 1 : 0, t->skip_probs[svt_nb_skip(a) + svt_nb_skip(lf)]);
        out[n + 1] = SVT_BOOL_RECORD(inter, t->intra_inter_prob[svt_mii_ctx_intra_inter(a, lf)]);
    }
    n += 2;
    if (!inter) { /* the luma mode(s) under the block's size group (0 for each of four 4x4 blocks), the chroma mode under the (last) luma mode */
        const uint8_t *yp = out ? t->y_mode_prob[ty == 0 ? 0 : l < 2 ? l + 1 : 3] : (const uint8_t *)0;
        for (int k = 0; k < (ty ? 1 : 4); k++) n += svt_mi_mode_bools(svt_mi_y_mode(b, k), yp, out ? out + n : (uint16_t *)0);
        n += svt_mi_mode_bools(b->pad_[2], out ? t->uv_mode_prob[svt_mi_y_mode(b, 3)] : (const uint8_t *)0, out ? out + n : (uint16_t *)0);
        return n;
    }
    const svt_mi_inter_ext *x = &v->ext[idx];
    const svt_mc_mode_info *m = &v->mc[idx];
    const int               comp = x->ref_frame[1] > 0;
    /* write_ref_frames */
    if (v->f.reference_mode == SVT_MODES_REFERENCE_SELECT) {
        if (out) out[n] = SVT_BOOL_RECORD(comp, t->comp_inter_prob[svt_mii_ctx_comp_inter(a, lf, v->f.comp_fixed_ref)]);
        n++;
    }
    if (comp) {
        if (out) {
            const int var_idx = !v->f.ref_frame_sign_bias[v->f.comp_fixed_ref & 3];
            out[n] = SVT_BOOL_RECORD(x->ref_frame[var_idx] == v->f.comp_var_ref[1], t->comp_ref_prob[svt_mii_ctx_comp_ref(a, lf, &v->f)]);
        }
        n++;
    } else {
        if (out) out[n] = SVT_BOOL_RECORD(x->ref_frame[0] != 1, t->single_ref_prob[svt_mii_ctx_single_p1(a, lf)][0]);
        n++;
        if (x->ref_frame[0] != 1) {
            if (out) out[n] = SVT_BOOL_RECORD(x->ref_frame[0] != 2, t->single_ref_prob[svt_mii_ctx_single_p2(a, lf)][1]);
            n++;
        }
    }
    /* the inter mode: leaves of the tree in the order ZEROMV, NEARESTMV, NEARMV, NEWMV */
    n += svt_mii_tree4(x->mode == 12 ? 0 : x->mode == 13 ? 3 : x->mode - 9, out ? t->inter_mode_probs[x->mode_context] : (const uint8_t *)0, out ? out + n : (uint16_t *)0);
    if (x->mode == 13)
        for (int k = 0; k <= comp; k++) {
            const int usehp = v->f.allow_hp && svt_mii_use_mv_hp(x->ref_mv_row[k], x->ref_mv_col[k]);
            n += svt_mii_mv_bools(m->mv_row[k] - x->ref_mv_row[k], m->mv_col[k] - x->ref_mv_col[k], usehp, t, out ? out + n : (uint16_t *)0);
        }
    return n;
}

#endif /* SVT_MODEINFO_INTER_CORE_H */
