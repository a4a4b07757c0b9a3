/*
 * ref_modes_driver.c -- runs the REFERENCE's key-frame tile coding and writes what it produced: per SB in raster order a depth-first
 * walk of the quad-tree that calls the reference's write_partition, write_mb_modes_kf, pack_mb_tokens and update_partition_context
 * (VPX/vp9_bitstream.c, VPX/vp9_onyxc_int.h) between eb_vp9_start_encode and eb_vp9_stop_encode, the way
 * Codec/EbEntropyCodingProcess.c:60-449 drives them: above partition context cleared once per picture, left partition context at the
 * first SB of an SB row, above_mi / left_mi NULL in picture row 0 / column 0.  Compiled by tests/gen_golden_modes.py against the
 * reference's headers and linked with the reference's own objects; the translation units the oracle's object set lacks are compiled
 * into this one by the includes below (write_mb_modes_kf and pack_mb_tokens are static there).  Nothing of the reference is copied here.
 *
 * request : int32 magic, n_pics; per picture int32 width, height, n_tokens; mi_rows * mi_cols records {uint8 sb_type, tx_size, skip,
 *           is_inter, filter_level, pad[3]} (modes: pad[1] luma or blocks 0, 1 in its nibbles, pad[0] blocks 2, 3, pad[2] chroma);
 *           n_tokens x {int32 token, extra, prob_row}; mi_rows * mi_cols x 6 int32 {first, count} of the Y, Cb, Cr token runs of the
 *           leaf whose origin the unit is
 * response: kf_y_mode_prob[900], kf_uv_mode_prob[90], kf_partition_probs[48], skip_probs[3], coef_probs[576 * 3], pareto[255 * 8],
 *           cat_probs[6 * 14] (uint8); per picture uint32 size, the tile's bytes, uint32 size, the bytes of the mode-info bools alone
 *           (the same walk without pack_mb_tokens), double seconds of one pass of the whole tile (the best of REPEAT)
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
#include "vp9_bitstream.c"

#define REPEAT 20

typedef struct {
    VP9_COMMON  *cm;
    MACROBLOCKD *xd;
    VpxWriter    w;
    TOKENEXTRA  *tok;       /* the picture's records */
    TOKENEXTRA  *leaf;      /* one leaf's records + EOSB */
    const int32_t *runs;    /* 6 per unit */
    int          with_tokens;
} drv;

static double drv_now(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

static void code_node(drv *d, int mi_row, int mi_col, BLOCK_SIZE bsize) {
    VP9_COMMON *cm = d->cm;
    MACROBLOCKD *xd = d->xd;
    if (mi_row >= cm->mi_rows || mi_col >= cm->mi_cols) return;
    const int bs = eb_vp9_num_8x8_blocks_wide_lookup[bsize], hbs = bs / 2;
    ModeInfo **at = cm->mi_grid_visible + mi_row * cm->mi_stride + mi_col;
    const PARTITION_TYPE partition = at[0]->sb_type == bsize ? PARTITION_NONE : PARTITION_SPLIT;
    const BLOCK_SIZE subsize = get_subsize(bsize, partition);
    xd->mi = at;
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
    write_mb_modes_kf(cm, xd, &d->w);
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

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[2];
    if (fread(hdr, 4, 2, f) != 2 || hdr[0] != 0x45444f4d) return 4;
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 5;

    VP9_COMMON  *cm = calloc(1, sizeof *cm);
    MACROBLOCKD *xd = calloc(1, sizeof *xd);
    cm->fc = calloc(1, sizeof *cm->fc);
    cm->frame_type = KEY_FRAME;
    cm->tx_mode = ALLOW_32X32;
    eb_vp9_init_mode_probs(cm->fc);
    eb_vp9_default_coef_probs(cm);
    const vpx_prob *prob_base = &cm->fc->coef_probs[0][0][0][0][0][0];
    if (sizeof eb_vp9_kf_y_mode_prob != 900 || sizeof eb_vp9_kf_uv_mode_prob != 90 || sizeof eb_vp9_kf_partition_probs != 48 || sizeof cm->fc->skip_probs != 3 ||
        sizeof cm->fc->coef_probs != 576 * 3 || sizeof eb_vp9_pareto8_full != 255 * 8)
        return 6;
    fwrite(eb_vp9_kf_y_mode_prob, 1, 900, out);
    fwrite(eb_vp9_kf_uv_mode_prob, 1, 90, out);
    fwrite(eb_vp9_kf_partition_probs, 1, 48, out);
    fwrite(cm->fc->skip_probs, 1, 3, out);
    fwrite(prob_base, 1, 576 * 3, out);
    fwrite(eb_vp9_pareto8_full, 1, 255 * 8, out);
    for (int t = CATEGORY1_TOKEN; t <= CATEGORY6_TOKEN; t++) {
        uint8_t row[14] = {0};
        if (eb_vp9_extra_bits[t].len > 14) return 7;
        memcpy(row, eb_vp9_extra_bits[t].prob, (size_t)eb_vp9_extra_bits[t].len);
        fwrite(row, 1, 14, out);
    }

    for (int k = 0; k < hdr[1]; k++) {
        int32_t whn[3];
        if (fread(whn, 4, 3, f) != 3 || whn[0] < 8 || whn[1] < 8 || (whn[0] & 7) || (whn[1] & 7) || whn[2] < 0) return 8;
        const int mi_rows = whn[1] >> 3, mi_cols = whn[0] >> 3, units = mi_rows * mi_cols, n_tok = whn[2];
        uint8_t  *grid = malloc((size_t)units * 8);
        int32_t  *rec = malloc(12 * (size_t)(n_tok + 1)), *runs = malloc(24 * (size_t)units);
        if (fread(grid, 8, (size_t)units, f) != (size_t)units || fread(rec, 12, (size_t)n_tok, f) != (size_t)n_tok || fread(runs, 24, (size_t)units, f) != (size_t)units)
            return 9;
        cm->mi_rows = mi_rows; cm->mi_cols = mi_cols; cm->mi_stride = mi_cols;
        ModeInfo  *blocks = calloc((size_t)units, sizeof *blocks);
        ModeInfo **vis = calloc((size_t)units, sizeof *vis);
        cm->mi_grid_visible = vis;
        cm->above_seg_context = calloc((size_t)mi_cols_aligned_to_sb(mi_cols), sizeof *cm->above_seg_context);
        xd->above_seg_context = cm->above_seg_context;
        /* every unit of a block points at the block's ModeInfo: the one at its origin */
        for (int r = 0; r < mi_rows; r++)
            for (int c = 0; c < mi_cols; c++) {
                const uint8_t *g = grid + 8 * (r * mi_cols + c);
                const int      n = eb_vp9_num_8x8_blocks_wide_lookup[g[0]], r0 = r & ~(n - 1), c0 = c & ~(n - 1);
                ModeInfo      *m = &blocks[r0 * mi_cols + c0];
                vis[r * mi_cols + c] = m;
                if (r != r0 || c != c0) continue;
                m->sb_type = (BLOCK_SIZE)g[0]; m->tx_size = (TX_SIZE)g[1]; m->skip = g[2];
                m->ref_frame[0] = INTRA_FRAME; m->ref_frame[1] = NONE;
                m->uv_mode = (PREDICTION_MODE)g[7];
                if (g[0] < BLOCK_8X8) {
                    m->bmi[0].as_mode = (PREDICTION_MODE)(g[6] & 15); m->bmi[1].as_mode = (PREDICTION_MODE)(g[6] >> 4);
                    m->bmi[2].as_mode = (PREDICTION_MODE)(g[5] & 15); m->bmi[3].as_mode = (PREDICTION_MODE)(g[5] >> 4);
                    m->mode = m->bmi[3].as_mode; /* the mode decision leaves the last quadrant's (Codec/EbEncDecProcess.c:2208-2212) */
                } else m->mode = (PREDICTION_MODE)g[6];
            }
        TOKENEXTRA *tok = calloc((size_t)n_tok + 1, sizeof *tok), *leaf = calloc((size_t)n_tok + 2, sizeof *leaf);
        for (int i = 0; i < n_tok; i++) {
            tok[i].token = (int16_t)rec[3 * i]; tok[i].extra = (int16_t)rec[3 * i + 1];
            tok[i].context_tree = prob_base + 3 * rec[3 * i + 2];
        }
        for (int u = 0; u < units; u++)
            for (int p = 0; p < 3; p++)
                if (runs[6 * u + 2 * p] < 0 || runs[6 * u + 2 * p + 1] < 0 || runs[6 * u + 2 * p] + runs[6 * u + 2 * p + 1] > n_tok) return 10;
        uint8_t *buf = malloc((size_t)n_tok * 24 + (size_t)units * 64 + 256);
        drv      d = {cm, xd, {0}, tok, leaf, runs, 1};
        double   best = 1e30;
        uint32_t size = 0;
        for (int rep = 0; rep < REPEAT; rep++) {
            const double t0 = drv_now();
            size = code_tile(&d, buf);
            const double dt = drv_now() - t0;
            best = dt < best ? dt : best;
        }
        fwrite(&size, 4, 1, out);
        fwrite(buf, 1, size, out);
        d.with_tokens = 0;
        size = code_tile(&d, buf);
        fwrite(&size, 4, 1, out);
        fwrite(buf, 1, size, out);
        fwrite(&best, 8, 1, out);
        free(buf); free(tok); free(leaf); free(blocks); free(vis); free(cm->above_seg_context); free(grid); free(rec); free(runs);
    }
    fclose(f);
    fclose(out);
    return 0;
}
