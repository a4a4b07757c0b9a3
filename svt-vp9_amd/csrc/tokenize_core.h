/*
 * tokenize_core.h -- the rules of coefficient tokenisation, written once as plain inline functions that compile both for the device
 * (csrc/tokenize.hip: the kernels call them) and for the host (host/tokenize_host.c: svt_hip_tokenize_picture and the scan tables),
 * like encdec_core.h.  No tables in memory except the scan order itself: token, extra bits, energy class, band and the two context
 * neighbours of a position are arithmetic.
 *
 *   svt_tok_position   one token of tokenize_b (VPX/vp9_tokenize.c:275-349): the record of scan position c of a block
 *   svt_tok_neighbors  the pair eb_vp9_scan_orders[ts][tt].neighbors holds for a raster position (VPX/vp9_scan.c)
 *   svt_tok_block_at   the transform block of a coded block that starts at a 4x4 unit of a plane -- what eb_vp9_tokenize_sb visits
 *                      (vp9_foreach_transformed_block, VPX/vp9_tokenize.c:397-430) -- with its entropy context
 *                      (get_entropy_context / eb_vp9_set_contexts, VPX/vp9_blockd.c) derived from the eob map instead of from
 *                      above / left context arrays that a serial walk keeps
 */
#ifndef SVT_TOKENIZE_CORE_H
#define SVT_TOKENIZE_CORE_H

#include <stdint.h>
#include "encdec_core.h"

/* VPX/vp9_tokenize.c:36-50, VPX/vp9_entropy.h:28-52: 0..4 -> the value; the categories are the octaves of |v| - 3 */
SVT_HD int svt_tok_token(int v) {
    const int a = v < 0 ? -v : v;
    const int oct = 35 - __builtin_clz((unsigned)(a - 3) | 1u); /* 4 + floor(log2(a - 3)) for a >= 5 */
    return a < 5 ? a : (oct < 10 ? oct : 10);
}
/* smallest |v| of a token: 0, 1, 2, 3, 4, 5, 7, 11, 19, 35, 67 */
SVT_HD int svt_tok_base(int tok) { return tok < 5 ? tok : 3 + (1 << (tok - 4)); }
/* eb_vp9_pt_energy_class[token] = {0,1,2,3,3,4,4,5,5,5,5,5}, straight from the value */
SVT_HD int svt_tok_energy(int v) {
    int a = v < 0 ? -v : v;
    a = a < 11 ? a : 11;
    return (int)((0x544444433210ull >> (4 * a)) & 0xf);
}
/* eb_vp9_coefband_trans_4x4 / _8x8plus (VPX/vp9_entropy.c) */
SVT_HD int svt_tok_band(int c, int ts) { return c == 0 ? 0 : c < 3 ? 1 : c < 6 ? 2 : c < 10 ? 3 : c < (ts == 0 ? 13 : 21) ? 4 : 5; }
/* eb_vp9_intra_mode_to_tx_type_lookup (VPX/vp9_reconintra.c:20-31); 0 for anything that is not a mode */
SVT_HD int svt_tok_intra_tx_type(int mode) { return mode > 9 ? 0 : (int)((0x3122130210ull >> (4 * mode)) & 3); }

/* The two earlier-scanned neighbours whose energy classes give the context of raster position p (not the first of the scan) of an
 * l x l block: above and left inside the block; the one that exists, twice, in row 0 / column 0; ADST_DCT (1) scans along rows and
 * takes the left one twice, DCT_ADST (2) the above one twice.  32x32 blocks have the default order only. */
SVT_HD void svt_tok_neighbors(int ts, int tt, int p, int *a, int *b) {
    const int l = 4 << ts, i = p >> (2 + ts), j = p & (l - 1);
    int na = p - l, nb = p - 1;
    if (i == 0) na = nb;
    else if (j == 0) nb = na;
    else if (ts < 3 && tt == 1) na = nb;
    else if (ts < 3 && tt == 2) nb = na;
    *a = na; *b = nb;
}

/* the record of scan position c (<= eob, < n) of a block: q = its coefficients (raster), scan = its scan order, ctx0 = the block's
 * entropy context.  Position eob of a block that is not full carries the EOB token with the band and context of that position. */
SVT_HD uint32_t svt_tok_position(const int16_t *q, const int16_t *scan, int c, int eob, int ts, int tt, int ptype, int inter, int ctx0) {
    int ctx = ctx0, tok = SVT_TOK_EOB, extra = 0;
    const int p = scan[c];
    if (c) {
        int a, b;
        svt_tok_neighbors(ts, tt, p, &a, &b);
        ctx = (1 + svt_tok_energy(q[a]) + svt_tok_energy(q[b])) >> 1;
    }
    if (c != eob) {
        const int v = q[p], m = v < 0 ? -v : v;
        tok = svt_tok_token(v);
        extra = tok ? (((m - svt_tok_base(tok)) << 1) | (v < 0)) & 0xffff : 0;
    }
    const int row = (((ts * 2 + ptype) * 2 + inter) * 6 + svt_tok_band(c, ts)) * 6 + ctx;
    return SVT_TOK_RECORD(extra, row, tok);
}

/* element offset of the {scan[n], neighbors[2 (n + 1)]} table of (tx_size, tx_type) in the canonical scan array */
SVT_HD int svt_tok_scan_offset(int ts, int tt) {
    int off = 0;
    for (int s = 0; s < ts; s++) off += 4 * (3 * (16 << (2 * s)) + 2);
    return off + tt * (3 * (16 << (2 * ts)) + 2);
}

/* ------------------------------------------------------------------------------------------------------------------------ */
/* transform blocks of a picture                                                                                              */
/* ------------------------------------------------------------------------------------------------------------------------ */
typedef struct svt_tok_geom {
    int mi_stride, mi_rows, mi_cols, w4, h4; /* w4 / h4: luma 4x4 units */
} svt_tok_geom;
typedef struct svt_tok_block {
    int ts, tt, inter, eob, ctx;
} svt_tok_block;
/* the pictures every grid stage takes: width / height 8 .. 8192 and a multiple of 8, mi_stride >= mi_cols.  0 and the geometry, the SBs
 * of a row and of the picture filled in; 1, nothing written, for any other picture */
SVT_HD int svt_tok_geom_of(int width, int height, int mi_stride, svt_tok_geom *g, int *sb_cols, int *n_sb) {
    if (width < 8 || height < 8 || width > 8192 || height > 8192 || (width & 7) || (height & 7) || mi_stride < (width >> 3)) return 1;
    g->mi_stride = mi_stride; g->mi_rows = height >> 3; g->mi_cols = width >> 3; g->w4 = width >> 2; g->h4 = height >> 2;
    *sb_cols = (width + 63) >> 6;
    *n_sb = *sb_cols * ((height + 63) >> 6);
    return 0;
}

SVT_HD int svt_tok_map_offset(const svt_tok_geom *g, int plane) {
    return plane == 0 ? 0 : g->w4 * g->h4 + (plane == 2 ? (g->w4 >> 1) * (g->h4 >> 1) : 0);
}
/* transform size of the block that covers the 4x4 unit (x4, y4) of a plane (units of that plane); -1: malformed record */
SVT_HD int svt_tok_ts_at(const svt_lf_mode_info *mi, const svt_tok_geom *g, int plane, int x4, int y4) {
    const svt_lf_mode_info *b = &mi[(plane ? y4 : y4 >> 1) * g->mi_stride + (plane ? x4 : x4 >> 1)];
    if (b->sb_type > 12 || b->tx_size > 3) return -1;
    return plane ? svt_uv_tx_size(b->sb_type, b->tx_size) : b->tx_size;
}
/* does the transform block that covers unit (x4, y4) have coefficients?  (a skipped block's entries of the eob map are all 0) */
SVT_HD int svt_tok_nz_at(const svt_lf_mode_info *mi, const uint16_t *eob_map, const svt_tok_geom *g, int plane, int x4, int y4) {
    const int ts = svt_tok_ts_at(mi, g, plane, x4, y4);
    if (ts < 0) return 0;
    const int m = (1 << ts) - 1, pw4 = plane ? g->w4 >> 1 : g->w4;
    return eob_map[svt_tok_map_offset(g, plane) + (y4 & ~m) * pw4 + (x4 & ~m)] != 0;
}
/* 1: a transform block of a coded block starts at unit (x4, y4) of the plane (inside the picture), *k describes it; 0: none does */
SVT_HD int svt_tok_block_at(const svt_lf_mode_info *mi, const uint16_t *eob_map, const svt_tok_geom *g, int plane, int x4, int y4, svt_tok_block *k) {
    const int pw4 = plane ? g->w4 >> 1 : g->w4, ph4 = plane ? g->h4 >> 1 : g->h4;
    if (x4 >= pw4 || y4 >= ph4) return 0;
    const svt_lf_mode_info *b = &mi[(plane ? y4 : y4 >> 1) * g->mi_stride + (plane ? x4 : x4 >> 1)];
    if (b->sb_type > 12 || b->tx_size > 3 || b->skip) return 0;
    const int ts = plane ? svt_uv_tx_size(b->sb_type, b->tx_size) : b->tx_size, s = 1 << ts;
    if ((x4 & (s - 1)) || (y4 & (s - 1)) || x4 + s > pw4 || y4 + s > ph4) return 0;
    int tt = 0;
    if (plane == 0 && ts < 3) {
        if (b->is_inter) tt = b->pad_[0] & 3;
        else if (b->sb_type == 0) { /* four 4x4 blocks: modes in the nibbles of pad_[1] (blocks 0, 1) and pad_[0] (blocks 2, 3) */
            const int q4 = (y4 & 1) * 2 + (x4 & 1);
            tt = svt_tok_intra_tx_type(((q4 < 2 ? b->pad_[1] : b->pad_[0]) >> (4 * (q4 & 1))) & 15);
        } else tt = svt_tok_intra_tx_type(b->pad_[1]);
    }
    int above = 0, left = 0;
    if (y4) for (int i = 0; i < s; i++) above |= svt_tok_nz_at(mi, eob_map, g, plane, x4 + i, y4 - 1);
    if (x4) for (int i = 0; i < s; i++) left |= svt_tok_nz_at(mi, eob_map, g, plane, x4 - 1, y4 + i);
    k->ts = ts; k->tt = tt; k->inter = b->is_inter ? 1 : 0; k->ctx = above + left;
    k->eob = eob_map[svt_tok_map_offset(g, plane) + y4 * pw4 + x4];
    if (k->eob > (16 << (2 * ts))) k->eob = 16 << (2 * ts);
    return 1;
}
SVT_HD int svt_tok_count(const svt_tok_block *k) { return k->eob + (k->eob < (16 << (2 * k->ts))); }
/* the 8x8 unit (row, column inside the SB) that is n-th in z-order */
SVT_HD void svt_tok_unit_of(int z, int *r, int *c) {
    *c = (z & 1) | (z >> 1 & 2) | (z >> 2 & 4);
    *r = (z >> 1 & 1) | (z >> 2 & 2) | (z >> 3 & 4);
}

#endif /* SVT_TOKENIZE_CORE_H */
