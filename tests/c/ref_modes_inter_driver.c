/*
 * ref_modes_inter_driver.c -- runs the REFERENCE's tile coding of inter pictures and writes what it produced: per SB in raster order a
 * depth-first walk of the quad-tree that calls the reference's write_partition, pack_inter_mode_mvs, pack_mb_tokens and
 * update_partition_context (VPX/vp9_bitstream.c, VPX/vp9_onyxc_int.h) between eb_vp9_start_encode and eb_vp9_stop_encode, the way
 * Codec/EbEntropyCodingProcess.c:60-449 drives them: above partition context cleared once per picture, left partition context at the
 * first SB of an SB row, above_mi / left_mi NULL in picture row 0 / column 0; comp_fixed_ref / comp_var_ref come from the reference's
 * eb_vp9_setup_compound_reference_mode.  Compiled by tests/gen_golden_modes_inter.py against the reference's headers and linked with
 * the reference's own objects; the translation units the oracle's object set lacks are compiled into this one by the includes below
 * (pack_inter_mode_mvs and pack_mb_tokens are static there).  Nothing of the reference is copied here.
 *
 * While it codes, the driver notes which contexts and symbols the reference met, with the reference's own context functions, so that
 * the generator can assert the fixture's coverage on the reference's side.
 *
 * request : int32 magic, n_pics; per picture int32 width, height, n_tokens, reference_mode, allow_hp, sign_bias[4]; mi_rows * mi_cols
 *           records {uint8 sb_type, tx_size, skip, is_inter, filter_level, pad[3]} (intra modes: pad[1] luma or blocks 0, 1 in its
 *           nibbles, pad[0] blocks 2, 3, pad[2] chroma); as many {int16 mv_row[2], mv_col[2]; int8 ref_list[2]; uint8 bw8, bh8}; as many
 *           {int16 ref_mv_row[2], ref_mv_col[2]; uint8 ref_frame[2], mode, mode_context}; n_tokens x {int32 token, extra, prob_row};
 *           mi_rows * mi_cols x 6 int32 {first, count} of the Y, Cb, Cr token runs of the leaf whose origin the unit is
 * response: fc's partition_prob[48], skip_probs[3], intra_inter_prob[4], comp_inter_prob[5], single_ref_prob[10], comp_ref_prob[5],
 *           y_mode_prob[36], uv_mode_prob[90], inter_mode_probs[21], nmvc[69], coef_probs[576 * 3], pareto[255 * 8], cat_probs[6 * 14]
 *           (uint8); per picture int32 comp_fixed_ref, comp_var_ref[2], uint32 size, the tile's bytes, uint32 size, the bytes of the
 *           mode-info bools alone (the same walk without pack_mb_tokens), double seconds of one pass of the whole tile (the best of
 *           REPEAT); then COV_WORDS uint32 of coverage masks (enum cov below)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <time.h>

#include "vpx_dsp_rtcd.h"
#include "vp9_rtcd.h"
#include "prob.c"
#include "bitwriter.c"
#include "vp9_entropymode.c"
#include "vp9_entropymv.c"
#include "vp9_encodemv.c"
#include "vp9_pred_common.c"
#include "vp9_bitstream.c"

#define REPEAT 20

enum cov { COV_PARTITION, COV_SKIP, COV_INTRA_INTER, COV_COMP_FLAG, COV_SINGLE_P1, COV_SINGLE_P2, COV_COMP_REF, COV_MODE, COV_MODE_CTX, COV_JOINT, COV_SIGN, COV_CLASS,
           COV_CLASS0_INT, COV_HP, COV_SIZE_GROUP, COV_REF_FRAME, COV_WORDS };

typedef struct {
    VP9_COMP      *cpi;
    VP9_COMMON    *cm;
    MACROBLOCKD   *xd;
    MbModeInfoExt *ext;       /* one per unit, read at a leaf's origin */
    VpxWriter      w;
    TOKENEXTRA    *tok;       /* the picture's records */
    TOKENEXTRA    *leaf;      /* one leaf's records + EOSB */
    const int32_t *runs;      /* 6 per unit */
    int            with_tokens;
    uint32_t      *cov;       /* NULL: do not note */
} drv;

static double drv_now(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

static void note_mv_component(uint32_t *cov, int comp, int usehp, int allow_hp) {
    int       offset;
    const int mag = comp < 0 ? -comp : comp, c = eb_vp9_get_mv_class(mag - 1, &offset);
    cov[COV_SIGN] |= 1u << (comp < 0);
    cov[COV_CLASS] |= 1u << c;
    if (c == MV_CLASS_0) cov[COV_CLASS0_INT] |= 1u << (offset >> 3);
    if (allow_hp) cov[COV_HP] |= 1u << (usehp != 0);
}

/* what the reference's context functions answer for the leaf xd points at, where pack_inter_mode_mvs codes under them */
static void note_leaf(drv *d, const MbModeInfoExt *ext) {
    const VP9_COMMON *cm = d->cm;
    const ModeInfo   *mi = d->xd->mi[0];
    uint32_t         *cov = d->cov;
    cov[COV_SKIP] |= 1u << vp9_get_skip_context(d->xd);
    cov[COV_INTRA_INTER] |= 1u << get_intra_inter_context(d->xd);
    if (!is_inter_block(mi)) {
        cov[COV_SIZE_GROUP] |= 1u << (mi->sb_type < BLOCK_8X8 ? 0 : eb_vp9_size_group_lookup[mi->sb_type]);
        return;
    }
    if (cm->reference_mode == REFERENCE_MODE_SELECT) cov[COV_COMP_FLAG] |= 1u << eb_vp9_get_reference_mode_context(cm, d->xd);
    if (has_second_ref(mi)) cov[COV_COMP_REF] |= 1u << eb_vp9_get_pred_context_comp_ref_p(cm, d->xd);
    else {
        cov[COV_SINGLE_P1] |= 1u << eb_vp9_get_pred_context_single_ref_p1(d->xd);
        if (mi->ref_frame[0] != LAST_FRAME) cov[COV_SINGLE_P2] |= 1u << eb_vp9_get_pred_context_single_ref_p2(d->xd);
        cov[COV_REF_FRAME] |= 1u << mi->ref_frame[0];
    }
    cov[COV_MODE] |= 1u << INTER_OFFSET(mi->mode);
    cov[COV_MODE_CTX] |= 1u << ext->mode_context[mi->ref_frame[0]];
    if (mi->mode == NEWMV)
        for (int ref = 0; ref < 1 + has_second_ref(mi); ref++) {
            const MV *r = &ext->ref_mvs[mi->ref_frame[ref]][0].as_mv;
            const MV  diff = {mi->mv[ref].as_mv.row - r->row, mi->mv[ref].as_mv.col - r->col};
            const int usehp = cm->allow_high_precision_mv && use_mv_hp(r);
            cov[COV_JOINT] |= 1u << vp9_get_mv_joint(&diff);
            if (diff.row) note_mv_component(cov, diff.row, usehp, cm->allow_high_precision_mv);
            if (diff.col) note_mv_component(cov, diff.col, usehp, cm->allow_high_precision_mv);
        }
}

static void code_node(drv *d, int mi_row, int mi_col, BLOCK_SIZE bsize) {
    VP9_COMMON  *cm = d->cm;
    MACROBLOCKD *xd = d->xd;
    if (mi_row >= cm->mi_rows || mi_col >= cm->mi_cols) return;
    const int bs = eb_vp9_num_8x8_blocks_wide_lookup[bsize], hbs = bs / 2;
    ModeInfo **at = cm->mi_grid_visible + mi_row * cm->mi_stride + mi_col;
    const PARTITION_TYPE partition = at[0]->sb_type == bsize ? PARTITION_NONE : PARTITION_SPLIT;
    const BLOCK_SIZE subsize = get_subsize(bsize, partition);
    xd->mi = at;
    if (d->cov && (mi_row + hbs < cm->mi_rows || mi_col + hbs < cm->mi_cols)) d->cov[COV_PARTITION] |= 1u << partition_plane_context(xd, mi_row, mi_col, bsize);
    write_partition(cm, xd, hbs, mi_row, mi_col, partition, bsize, &d->w);
    if (partition == PARTITION_SPLIT && bsize != BLOCK_8X8) {
        code_node(d, mi_row, mi_col, subsize);
        code_node(d, mi_row, mi_col + hbs, subsize);
        code_node(d, mi_row + hbs, mi_col, subsize);
        code_node(d, mi_row + hbs, mi_col + hbs, subsize);
        return;
    }
    xd->above_mi = mi_row > 0 ? at[-cm->mi_stride] : NULL;
    xd->left_mi = mi_col > 0 ? at[-1] : NULL;
    const MbModeInfoExt *ext = d->ext + mi_row * cm->mi_cols + mi_col;
    unsigned int         max_mv_magnitude = 0;
    if (d->cov) note_leaf(d, ext);
    pack_inter_mode_mvs(d->cpi, xd, ext, &d->w, &max_mv_magnitude);
    if (d->with_tokens) {
        const int32_t *run = d->runs + 6 * (mi_row * cm->mi_cols + mi_col);
        TOKENEXTRA    *t = d->leaf;
        for (int p = 0; p < 3; p++) {
            memcpy(t, d->tok + run[2 * p], sizeof *t * (size_t)run[2 * p + 1]);
            t += run[2 * p + 1];
        }
        t->token = EOSB_TOKEN;
        TOKENEXTRA *tp = d->leaf;
        pack_mb_tokens(&d->w, &tp, t + 1, VPX_BITS_8);
        if (tp != t + 1) exit(20);
    }
    update_partition_context(xd, mi_row, mi_col, subsize, bsize);
}

static uint32_t code_tile(drv *d, uint8_t *buf) {
    VP9_COMMON *cm = d->cm;
    eb_vp9_start_encode(&d->w, buf);
    memset(cm->above_seg_context, 0, (size_t)mi_cols_aligned_to_sb(cm->mi_cols));
    for (int mi_row = 0; mi_row < cm->mi_rows; mi_row += MI_BLOCK_SIZE) {
        memset(d->xd->left_seg_context, 0, sizeof d->xd->left_seg_context);
        set_partition_probs(cm, d->xd);
        for (int mi_col = 0; mi_col < cm->mi_cols; mi_col += MI_BLOCK_SIZE) code_node(d, mi_row, mi_col, BLOCK_64X64);
    }
    eb_vp9_stop_encode(&d->w);
    return d->w.pos;
}

typedef struct { int16_t mv_row[2], mv_col[2]; int8_t ref_list[2]; uint8_t bw8, bh8; } mc_rec;
typedef struct { int16_t ref_mv_row[2], ref_mv_col[2]; uint8_t ref_frame[2], mode, mode_context; } ext_rec;

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[2];
    if (fread(hdr, 4, 2, f) != 2 || hdr[0] != 0x49444f4d) return 4;
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 5;

    VP9_COMP    *cpi = calloc(1, sizeof *cpi);
    VP9_COMMON  *cm = &cpi->common;
    MACROBLOCKD *xd = calloc(1, sizeof *xd);
    uint32_t     cov[COV_WORDS] = {0};
    cm->fc = calloc(1, sizeof *cm->fc);
    cm->frame_type = INTER_FRAME;
    cm->intra_only = 0;
    cm->tx_mode = ALLOW_32X32;
    eb_vp9_init_mode_probs(cm->fc);
    eb_vp9_init_mv_probs(cm);
    eb_vp9_default_coef_probs(cm);
    eb_vp9_entropy_mv_init();
    const FRAME_CONTEXT *fc = cm->fc;
    const vpx_prob      *prob_base = &fc->coef_probs[0][0][0][0][0][0];
    if (sizeof fc->partition_prob != 48 || sizeof fc->skip_probs != 3 || sizeof fc->intra_inter_prob != 4 || sizeof fc->comp_inter_prob != 5 ||
        sizeof fc->single_ref_prob != 10 || sizeof fc->comp_ref_prob != 5 || sizeof fc->y_mode_prob != 36 || sizeof fc->uv_mode_prob != 90 ||
        sizeof fc->inter_mode_probs != 21 || sizeof fc->nmvc != 69 || sizeof fc->coef_probs != 576 * 3 || sizeof eb_vp9_pareto8_full != 255 * 8 ||
        sizeof(mc_rec) != 12 || sizeof(ext_rec) != 12)
        return 6;
    fwrite(fc->partition_prob, 1, 48, out);
    fwrite(fc->skip_probs, 1, 3, out);
    fwrite(fc->intra_inter_prob, 1, 4, out);
    fwrite(fc->comp_inter_prob, 1, 5, out);
    fwrite(fc->single_ref_prob, 1, 10, out);
    fwrite(fc->comp_ref_prob, 1, 5, out);
    fwrite(fc->y_mode_prob, 1, 36, out);
    fwrite(fc->uv_mode_prob, 1, 90, out);
    fwrite(fc->inter_mode_probs, 1, 21, out);
    fwrite(&fc->nmvc, 1, 69, out);
    fwrite(prob_base, 1, 576 * 3, out);
    fwrite(eb_vp9_pareto8_full, 1, 255 * 8, out);
    for (int t = CATEGORY1_TOKEN; t <= CATEGORY6_TOKEN; t++) {
        uint8_t row[14] = {0};
        if (eb_vp9_extra_bits[t].len > 14) return 7;
        memcpy(row, eb_vp9_extra_bits[t].prob, (size_t)eb_vp9_extra_bits[t].len);
        fwrite(row, 1, 14, out);
    }

    for (int k = 0; k < hdr[1]; k++) {
        int32_t whn[9];
        if (fread(whn, 4, 9, f) != 9 || whn[0] < 8 || whn[1] < 8 || (whn[0] & 7) || (whn[1] & 7) || whn[2] < 0 || whn[3] < 0 || whn[3] > 2) return 8;
        const int mi_rows = whn[1] >> 3, mi_cols = whn[0] >> 3, units = mi_rows * mi_cols, n_tok = whn[2];
        uint8_t  *grid = malloc((size_t)units * 8);
        mc_rec   *mc = malloc(sizeof *mc * (size_t)units);
        ext_rec  *er = malloc(sizeof *er * (size_t)units);
        int32_t  *rec = malloc(12 * (size_t)(n_tok + 1)), *runs = malloc(24 * (size_t)units);
        if (fread(grid, 8, (size_t)units, f) != (size_t)units || fread(mc, 12, (size_t)units, f) != (size_t)units || fread(er, 12, (size_t)units, f) != (size_t)units ||
            fread(rec, 12, (size_t)n_tok, f) != (size_t)n_tok || fread(runs, 24, (size_t)units, f) != (size_t)units)
            return 9;
        cm->mi_rows = mi_rows; cm->mi_cols = mi_cols; cm->mi_stride = mi_cols;
        cm->reference_mode = (REFERENCE_MODE)whn[3];
        cm->allow_high_precision_mv = whn[4];
        for (int i = 0; i < 4; i++) cm->ref_frame_sign_bias[i] = whn[5 + i];
        eb_vp9_setup_compound_reference_mode(cm);
        ModeInfo      *blocks = calloc((size_t)units, sizeof *blocks);
        ModeInfo     **vis = calloc((size_t)units, sizeof *vis);
        MbModeInfoExt *ext = calloc((size_t)units, sizeof *ext);
        cm->mi_grid_visible = vis;
        cm->above_seg_context = calloc((size_t)mi_cols_aligned_to_sb(mi_cols), sizeof *cm->above_seg_context);
        xd->above_seg_context = cm->above_seg_context;
        /* every unit of a block points at the block's ModeInfo: the one at its origin */
        for (int r = 0; r < mi_rows; r++)
            for (int c = 0; c < mi_cols; c++) {
                const int      u = r * mi_cols + c;
                const uint8_t *g = grid + 8 * u;
                const int      n = eb_vp9_num_8x8_blocks_wide_lookup[g[0]], r0 = r & ~(n - 1), c0 = c & ~(n - 1);
                ModeInfo      *m = &blocks[r0 * mi_cols + c0];
                vis[u] = m;
                if (r != r0 || c != c0) continue;
                m->sb_type = (BLOCK_SIZE)g[0]; m->tx_size = (TX_SIZE)g[1]; m->skip = g[2];
                if (!g[3]) {
                    m->ref_frame[0] = INTRA_FRAME; m->ref_frame[1] = NONE;
                    m->uv_mode = (PREDICTION_MODE)g[7];
                    if (g[0] < BLOCK_8X8) {
                        m->bmi[0].as_mode = (PREDICTION_MODE)(g[6] & 15); m->bmi[1].as_mode = (PREDICTION_MODE)(g[6] >> 4);
                        m->bmi[2].as_mode = (PREDICTION_MODE)(g[5] & 15); m->bmi[3].as_mode = (PREDICTION_MODE)(g[5] >> 4);
                        m->mode = m->bmi[3].as_mode; /* the mode decision leaves the last quadrant's (Codec/EbEncDecProcess.c:2208-2212) */
                    } else m->mode = (PREDICTION_MODE)g[6];
                    continue;
                }
                m->ref_frame[0] = (MV_REFERENCE_FRAME)er[u].ref_frame[0];
                m->ref_frame[1] = er[u].ref_frame[1] ? (MV_REFERENCE_FRAME)er[u].ref_frame[1] : NONE;
                m->mode = (PREDICTION_MODE)er[u].mode;
                for (int ref = 0; ref < 2; ref++) {
                    m->mv[ref].as_mv.row = mc[u].mv_row[ref]; m->mv[ref].as_mv.col = mc[u].mv_col[ref];
                    if (ref && !er[u].ref_frame[1]) break;
                    ext[u].ref_mvs[er[u].ref_frame[ref]][0].as_mv.row = er[u].ref_mv_row[ref];
                    ext[u].ref_mvs[er[u].ref_frame[ref]][0].as_mv.col = er[u].ref_mv_col[ref];
                }
                ext[u].mode_context[er[u].ref_frame[0]] = er[u].mode_context;
            }
        TOKENEXTRA *tok = calloc((size_t)n_tok + 1, sizeof *tok), *leaf = calloc((size_t)n_tok + 2, sizeof *leaf);
        for (int i = 0; i < n_tok; i++) {
            tok[i].token = (int16_t)rec[3 * i]; tok[i].extra = (int16_t)rec[3 * i + 1];
            tok[i].context_tree = prob_base + 3 * rec[3 * i + 2];
        }
        for (int u = 0; u < units; u++)
            for (int p = 0; p < 3; p++)
                if (runs[6 * u + 2 * p] < 0 || runs[6 * u + 2 * p + 1] < 0 || runs[6 * u + 2 * p] + runs[6 * u + 2 * p + 1] > n_tok) return 10;
        uint8_t *buf = malloc((size_t)n_tok * 24 + (size_t)units * 256 + 256);
        drv      d = {cpi, cm, xd, ext, {0}, tok, leaf, runs, 1, NULL};
        double   best = 1e30;
        uint32_t size = 0;
        for (int rep = 0; rep < REPEAT; rep++) {
            const double t0 = drv_now();
            size = code_tile(&d, buf);
            const double dt = drv_now() - t0;
            best = dt < best ? dt : best;
        }
        const int32_t refs[3] = {cm->comp_fixed_ref, cm->comp_var_ref[0], cm->comp_var_ref[1]};
        fwrite(refs, 4, 3, out);
        fwrite(&size, 4, 1, out);
        fwrite(buf, 1, size, out);
        d.with_tokens = 0;
        d.cov = cov;
        size = code_tile(&d, buf);
        fwrite(&size, 4, 1, out);
        fwrite(buf, 1, size, out);
        fwrite(&best, 8, 1, out);
        free(buf); free(tok); free(leaf); free(blocks); free(vis); free(ext); free(cm->above_seg_context); free(grid); free(mc); free(er); free(rec); free(runs);
    }
    fwrite(cov, 4, COV_WORDS, out);
    fclose(f);
    fclose(out);
    return 0;
}
