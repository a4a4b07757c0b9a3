/*
 * modeinfo_core.h -- the rules of the key-frame mode-info syntax, written once as plain inline functions that compile both for the
 * device (csrc/modeinfo.hip) and for the host (host/modeinfo_host.c), like tokenize_core.h and boolcode_core.h.
 *
 * What the reference codes per block in front of its tokens (Codec/EbEntropyCodingProcess.c:110-442 over write_partition,
 * VPX/vp9_bitstream.c:399-417, and write_mb_modes_kf, :323-358), as raw bool records for the bool coder's kind-1 segments.  The
 * serial walk keeps above / left arrays (above_seg_context, left_seg_context, above_mi, left_mi); here every context is read from
 * the grid: the leaf above (r - 1, c) and the leaf left (r, c - 1) of a node's origin (r, c) are coded in front of the node, and
 * nothing coded between them and the node touches column c of the above array or row r of the left array.  So the partition context
 * is partition_context_lookup[] of those two records' sb_type (0 in picture row 0 / column 0: the above array is cleared once per
 * picture, the left array per SB row), the skip context is their skip flags, the luma mode context their luma modes.
 *
 *   svt_mi_check        is the record of an 8x8 unit one this syntax takes?
 *   svt_mi_mode_bools   one intra mode through eb_vp9_intra_mode_tree (VPX/vp9_entropymode.c)
 *   svt_mi_unit_bools   the bools that start at an 8x8 unit: the partition symbols of every node whose origin it is, outermost first,
 *                       then -- the unit is a leaf's origin -- skip, luma mode(s), chroma mode
 *   svt_mi_leaf_tokens  first token and token count of a leaf's Y, Cb and Cr runs in the tokeniser's output
 */
#ifndef SVT_MODEINFO_CORE_H
#define SVT_MODEINFO_CORE_H

#include <stdint.h>
#include "tokenize_core.h"

/* The longest path of the mode tree has 7 nodes (D153, D207); a partition symbol has at most 3 bools (SPLIT) and a unit is the origin
 * of at most 4 nodes (64, 32, 16, 8): 4 * 3 + skip + 4 luma modes * 7 + chroma mode * 7 */
#define SVT_MI_MODE_BOOLS 7
#define SVT_MI_UNIT_BOOLS (4 * 3 + 1 + 4 * SVT_MI_MODE_BOOLS + SVT_MI_MODE_BOOLS)

/* log2 of a square block's side in 8x8 units: sb_type 0 (four 4x4 blocks) and 3 -> 0, 6 -> 1, 9 -> 2, 12 -> 3 */
SVT_HD int svt_mi_level(int sb_type) { return sb_type ? sb_type / 3 - 1 : 0; }
/* partition_context_lookup[sb_type] (VPX/vp9_onyxc_int.h:63-77) of the square sizes: 15, 14, 12, 8, 0 -- bit L says "smaller than a node of level L" */
SVT_HD int svt_mi_seg_context(int sb_type) { return (15 << ((sb_type / 3) & 7)) & 15; }
/* luma mode of block k (0 .. 3) of a record: get_y_mode (VPX/vp9_blockd.h:100-102) */
SVT_HD int svt_mi_y_mode(const svt_lf_mode_info *b, int k) {
    return b->sb_type ? b->pad_[1] : ((k < 2 ? b->pad_[1] : b->pad_[0]) >> (4 * (k & 1))) & 15;
}

/* 0: the unit (r, c) lies in a block this syntax takes -- square, intra, modes 0 .. 9, inside the picture, transform = the block's
 * largest up to 32x32, and no enclosing node's origin claims a larger block */
SVT_HD int svt_mi_check(const svt_lf_mode_info *mi, const svt_tok_geom *g, int r, int c) {
    const svt_lf_mode_info *b = &mi[r * g->mi_stride + c];
    const int t = b->sb_type;
    if (t > 12 || t % 3 || b->is_inter || b->pad_[2] > 9) return 1;
    const int l = svt_mi_level(t), n = 1 << l;
    if ((r & ~(n - 1)) + n > g->mi_rows || (c & ~(n - 1)) + n > g->mi_cols) return 1;
    if (b->tx_size != (t == 0 ? 0 : l < 2 ? l + 1 : 3)) return 1;
    for (int k = 0; k < (t ? 1 : 4); k++)
        if (svt_mi_y_mode(b, k) > 9) return 1;
    for (int L = l; L <= 3; L++) { /* the origin of the enclosing node of level L: this block's own (L = l), or a smaller block's */
        const int m = (1 << L) - 1, to = mi[(r & ~m) * g->mi_stride + (c & ~m)].sb_type;
        if (to > 12 || to % 3 || (L == l ? to != t : svt_mi_level(to) >= L)) return 1;
    }
    return 0;
}

/* The tree in words: DC | (TM | (V | ((H | (D135 | D117)) | (D45 | (D63 | (D153 | D207)))))), node k's probability is probs[k] with the
 * nodes numbered top down, the H side (4, 5) in front of the D45 side (6, 7, 8).  A mode's path: its length, and its bits from the top. */
SVT_HD int svt_mi_mode_len(int mode) { return (int)((0x2677665531ull >> (4 * mode)) & 15); }
SVT_HD int svt_mi_mode_path(int mode) { return (int)((mode < 8 ? 0x7F7E3B3A1E1C0600ull >> (8 * mode) : 0x023Eull >> (8 * (mode - 8))) & 255); }
/* the bools of one mode (out may be NULL: the count alone) */
SVT_HD int svt_mi_mode_bools(int mode, const uint8_t *probs, uint16_t *out) {
    const int len = svt_mi_mode_len(mode), v = svt_mi_mode_path(mode);
    if (out) {
        const int d45_side = len > 3 && ((v >> (len - 4)) & 1); /* the fourth bool chooses the side: nodes 4, 5 or 6, 7, 8 */
        for (int k = 0; k < len; k++) out[k] = SVT_BOOL_RECORD((v >> (len - 1 - k)) & 1, probs[k < 4 ? k : k + 2 * d45_side]);
    }
    return len;
}

/* The bools that start at unit (r, c) of a well-formed grid, in coding order; 0 when the unit is no leaf's origin.  out (and t) may
 * be NULL: the count alone, which needs no probabilities.  At most SVT_MI_UNIT_BOOLS. */
SVT_HD int svt_mi_unit_bools(const svt_lf_mode_info *mi, const svt_tok_geom *g, int r, int c, const svt_modes_tables *t, uint16_t *out) {
    const svt_lf_mode_info *b = &mi[r * g->mi_stride + c], *ab = r ? b - g->mi_stride : (const svt_lf_mode_info *)0, *lb = c ? b - 1 : (const svt_lf_mode_info *)0;
    const int ty = b->sb_type, l = svt_mi_level(ty);
    if ((r | c) & ((1 << l) - 1)) return 0;
    int n = 0;
    /* write_partition at every node whose origin this is.  Only NONE and SPLIT occur; a node larger than the leaf is SPLIT, and so is
       the 8x8 node of four 4x4 blocks.  partition_tree: NONE = 0; SPLIT = 1 1 1 under probs[0 .. 2] */
    const int sa = ab ? svt_mi_seg_context(ab->sb_type) : 0, sl = lb ? svt_mi_seg_context(lb->sb_type) : 0;
    for (int L = 3; L >= l; L--) {
        if ((r | c) & ((1 << L) - 1)) continue;
        const int hbs = (1 << L) >> 1, has_rows = r + hbs < g->mi_rows, has_cols = c + hbs < g->mi_cols, split = L > l || ty == 0;
        const uint8_t *p = out ? t->kf_partition_probs[4 * L + 2 * ((sl >> L) & 1) + ((sa >> L) & 1)] : (const uint8_t *)0;
        if (has_rows && has_cols) {
            if (out) out[n] = SVT_BOOL_RECORD(split, p[0]);
            n++;
            if (split) {
                if (out) { out[n] = SVT_BOOL_RECORD(1, p[1]); out[n + 1] = SVT_BOOL_RECORD(1, p[2]); }
                n += 2;
            }
        } else if (has_rows || has_cols) { /* the half outside the picture is not coded: one bool says SPLIT (a node at the edge is never a leaf) */
            if (out) out[n] = SVT_BOOL_RECORD(1, p[has_cols ? 1 : 2]);
            n++;
        }
    }
    /* write_mb_modes_kf: skip; no transform size (tx_mode ALLOW_32X32), no segment id; the luma mode(s) under the modes above and left
       of each (DC where there is no neighbour; blocks 2, 3 of a 4x4 unit look at blocks 0, 1 of their own, blocks 1, 3 at 0, 2); the
       chroma mode under the unit's mi->mode, which for four 4x4 blocks is the last one's */
    if (out) out[n] = SVT_BOOL_RECORD(b->skip ? 1 : 0, t->skip_probs[(ab && ab->skip) + (lb && lb->skip)]);
    n++;
    const int a0 = ab ? svt_mi_y_mode(ab, 2) : 0, a1 = ab ? svt_mi_y_mode(ab, 3) : 0, l0 = lb ? svt_mi_y_mode(lb, 1) : 0, l2 = lb ? svt_mi_y_mode(lb, 3) : 0;
    if (ty) n += svt_mi_mode_bools(b->pad_[1], out ? t->kf_y_mode_prob[a0][l0] : (const uint8_t *)0, out ? out + n : (uint16_t *)0);
    else {
        const int m0 = svt_mi_y_mode(b, 0), m1 = svt_mi_y_mode(b, 1), m2 = svt_mi_y_mode(b, 2), m3 = svt_mi_y_mode(b, 3);
        n += svt_mi_mode_bools(m0, out ? t->kf_y_mode_prob[a0][l0] : (const uint8_t *)0, out ? out + n : (uint16_t *)0);
        n += svt_mi_mode_bools(m1, out ? t->kf_y_mode_prob[a1][m0] : (const uint8_t *)0, out ? out + n : (uint16_t *)0);
        n += svt_mi_mode_bools(m2, out ? t->kf_y_mode_prob[m0][l2] : (const uint8_t *)0, out ? out + n : (uint16_t *)0);
        n += svt_mi_mode_bools(m3, out ? t->kf_y_mode_prob[m1][m2] : (const uint8_t *)0, out ? out + n : (uint16_t *)0);
    }
    n += svt_mi_mode_bools(b->pad_[2], out ? t->kf_uv_mode_prob[svt_mi_y_mode(b, 3)] : (const uint8_t *)0, out ? out + n : (uint16_t *)0);
    return n;
}

/* The token runs of the leaf whose origin is unit (r, c): first[p] = first token, count[p] = tokens of plane p -- eob + (eob < n) per
 * transform block, as the tokeniser emits them; 0 / 0 for a skipped leaf.  A leaf's transform blocks of one plane are consecutive in the
 * tokeniser's order (z-order of their origins inside the SB's plane area). */
SVT_HD void svt_mi_leaf_tokens(const svt_lf_mode_info *mi, const uint16_t *eob_map, const uint32_t *tok_off, const svt_tok_geom *g, int r, int c, uint32_t *first,
                               uint32_t *count) {
    const svt_lf_mode_info *b = &mi[r * g->mi_stride + c];
    first[0] = first[1] = first[2] = 0;
    count[0] = count[1] = count[2] = 0;
    if (b->skip) return;
    const int ty = b->sb_type, ts = b->tx_size, n = 16 << (2 * ts), blocks = (ty == 0 || ty == 12) ? 4 : 1;
    for (int i = 0; i < blocks; i++) { /* four 4x4 blocks of a unit, four 32x32 blocks of a 64x64 leaf */
        const int e = eob_map[(2 * r + ((i >> 1) << ts)) * g->w4 + 2 * c + ((i & 1) << ts)];
        count[0] += (uint32_t)(e < n ? e + 1 : n);
    }
    first[0] = tok_off[2 * r * g->w4 + 2 * c];
    const int tu = svt_uv_tx_size(ty, ts), nu = 16 << (2 * tu);
    for (int p = 1; p < 3; p++) {
        const int idx = svt_tok_map_offset(g, p) + r * (g->w4 >> 1) + c, e = eob_map[idx];
        count[p] = (uint32_t)(e < nu ? e + 1 : nu);
        first[p] = tok_off[idx];
    }
}

#endif /* SVT_MODEINFO_CORE_H */
