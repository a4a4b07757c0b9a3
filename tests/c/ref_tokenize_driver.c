/*
 * ref_tokenize_driver.c -- runs the REFERENCE's eb_vp9_tokenize_sb (VPX/vp9_tokenize.c:397-430) over every block of a picture, in the
 * entropy coder's order and on a real MACROBLOCKD set up the way EntropyCodingSb sets it up (Codec/EbEntropyCodingProcess.c:88-105,
 * 146-214, 382-394), and writes what it produced.  Compiled by tests/gen_golden_tokens.py against the reference's headers and linked
 * with the reference's own objects; nothing of the reference is copied here.
 *
 * request : int32 magic, width, height; mi_rows * mi_cols records {sb_type, tx_size, skip, is_inter, filter_level, pad[3]} (the
 *           project's grid: luma modes / transform type in pad, see include/svtvp9_hip.h); n_sb * 6144 int16 coefficients in the
 *           project's position-addressed layout; the eob map (uint16, [Y][Cb][Cr] per 4x4 unit)
 * response: int32 n_blocks; per transform block int32 plane, x4, y4, n_tokens, then n_tokens x {int32 token, extra (low 16 bits),
 *           (context_tree - coef_probs base) / 3}; 6912 uint32 coef_counts; double seconds spent inside eb_vp9_tokenize_sb
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <time.h>

#include "vpx_dsp_rtcd.h"
#include "vp9_rtcd.h"
#include "vp9_encoder.h"
#include "vp9_tokenize.h"
#include "vp9_onyxc_int.h"

typedef struct { uint8_t sb_type, tx_size, skip, is_inter, filter_level, pad[3]; } grid_rec;

static uint32_t zorder4(int x, int y) {
    uint32_t v = 0;
    for (int b = 0; b < 4; b++) v |= (uint32_t)((x >> b) & 1) << (2 * b) | (uint32_t)((y >> b) & 1) << (2 * b + 1);
    return v;
}
/* element offset of the transform block at 4x4 unit (x4, y4) of a plane in the project's coefficient layout */
static size_t coeff_offset(int plane, int x4, int y4, int sb_cols) {
    const int u = plane ? 8 : 16;
    return (size_t)((y4 / u) * sb_cols + x4 / u) * 6144 + (plane == 0 ? 0 : plane == 1 ? 4096 : 5120) + zorder4(x4 % u, y4 % u) * 16;
}
static double now(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[3];
    if (fread(hdr, 4, 3, f) != 3 || hdr[0] != 0x4b4f5453) return 4;
    const int W = hdr[1], H = hdr[2], mi_rows = H / 8, mi_cols = W / 8, sb_cols = (W + 63) / 64, sb_rows = (H + 63) / 64, w4 = W / 4, h4 = H / 4;
    const size_t n_coeff = (size_t)sb_cols * sb_rows * 6144, n_map = (size_t)w4 * h4 * 3 / 2;
    grid_rec *grid = malloc(sizeof(grid_rec) * mi_rows * mi_cols);
    int16_t  *q = malloc(sizeof(int16_t) * n_coeff);
    uint16_t *emap = malloc(sizeof(uint16_t) * n_map);
    if (fread(grid, sizeof(grid_rec), (size_t)mi_rows * mi_cols, f) != (size_t)mi_rows * mi_cols || fread(q, 2, n_coeff, f) != n_coeff || fread(emap, 2, n_map, f) != n_map) return 5;
    fclose(f);
    const size_t map_off[3] = {0, (size_t)w4 * h4, (size_t)w4 * h4 + (size_t)(w4 / 2) * (h4 / 2)};

    /* the reference's objects */
    VP9_COMP    *cpi = calloc(1, sizeof *cpi);
    VP9_COMMON  *cm = &cpi->common;
    MACROBLOCKD *xd = calloc(1, sizeof *xd);
    cm->fc = calloc(1, sizeof *cm->fc);
    cm->mi_rows = mi_rows; cm->mi_cols = mi_cols; cm->mi_stride = mi_cols;
    cm->above_context = calloc((size_t)MAX_MB_PLANE * 2 * mi_cols_aligned_to_sb(mi_cols), sizeof *cm->above_context);
    cm->above_seg_context = calloc(mi_cols_aligned_to_sb(mi_cols), sizeof *cm->above_seg_context);
    ModeInfo  *mis = calloc((size_t)mi_rows * mi_cols, sizeof *mis);
    ModeInfo **mi_grid = calloc((size_t)mi_rows * mi_cols, sizeof *mi_grid);
    static const uint8_t w8_of[13] = {1, 1, 1, 1, 1, 2, 2, 2, 4, 4, 4, 8, 8}, h8_of[13] = {1, 1, 1, 1, 2, 1, 2, 4, 2, 4, 8, 4, 8};
    for (int r = 0; r < mi_rows; r++)
        for (int c = 0; c < mi_cols; c++) {
            const grid_rec *g = &grid[r * mi_cols + c];
            if (g->sb_type > 12) return 6;
            const int or_ = r - r % h8_of[g->sb_type], oc = c - c % w8_of[g->sb_type];
            mi_grid[r * mi_cols + c] = &mis[or_ * mi_cols + oc]; /* every unit of a block points at the block's ModeInfo */
            if (or_ != r || oc != c) continue;
            ModeInfo *m = &mis[r * mi_cols + c];
            m->sb_type = (BLOCK_SIZE)g->sb_type; m->tx_size = (TX_SIZE)g->tx_size; m->skip = (int8_t)g->skip;
            m->ref_frame[0] = g->is_inter ? LAST_FRAME : INTRA_FRAME; m->ref_frame[1] = NONE;
            if (g->is_inter) m->mode = ZEROMV;
            else if (g->sb_type == 0) {
                m->bmi[0].as_mode = (PREDICTION_MODE)(g->pad[1] & 15); m->bmi[1].as_mode = (PREDICTION_MODE)(g->pad[1] >> 4);
                m->bmi[2].as_mode = (PREDICTION_MODE)(g->pad[0] & 15); m->bmi[3].as_mode = (PREDICTION_MODE)(g->pad[0] >> 4);
                m->mode = m->bmi[3].as_mode;
            } else m->mode = (PREDICTION_MODE)g->pad[1];
            m->uv_mode = (PREDICTION_MODE)g->pad[2];
        }
    cm->mi_grid_visible = mi_grid;

    int16_t    *blk_q[3];
    uint16_t   *blk_eob[3];
    for (int p = 0; p < 3; p++) { blk_q[p] = calloc(64 * 64, sizeof(int16_t)); blk_eob[p] = calloc(256, sizeof(uint16_t)); }
    TOKENEXTRA *tok = calloc(64 * 64 * 3 + 1024, sizeof *tok);
    FILE       *out = fopen(argv[2], "wb");
    if (!out) return 7;
    int32_t n_blocks = 0;
    fwrite(&n_blocks, 4, 1, out);
    double  spent = 0;
    const vpx_prob *prob_base = &cm->fc->coef_probs[0][0][0][0][0][0];

    for (int sb = 0; sb < sb_rows * sb_cols; sb++) {
        const int sr = sb / sb_cols, sc = sb % sb_cols;
        if (sb == 0) memset(cm->above_context, 0, sizeof(*cm->above_context) * MAX_MB_PLANE * 2 * mi_cols_aligned_to_sb(cm->mi_cols));
        if (sc == 0) memset(&xd->left_context, 0, sizeof(xd->left_context));
        for (int z = 0; z < 64; z++) { /* blocks in coding order = z-order of their first 8x8 unit */
            int ur = 0, uc = 0;
            for (int b = 0; b < 3; b++) { uc |= ((z >> (2 * b)) & 1) << b; ur |= ((z >> (2 * b + 1)) & 1) << b; }
            const int mi_row = sr * 8 + ur, mi_col = sc * 8 + uc;
            if (mi_row >= mi_rows || mi_col >= mi_cols) continue;
            ModeInfo *m = mi_grid[mi_row * mi_cols + mi_col];
            if (m != &mis[mi_row * mi_cols + mi_col]) continue;
            const BLOCK_SIZE bsize = m->sb_type < BLOCK_8X8 ? BLOCK_8X8 : m->sb_type;
            xd->mi = &mi_grid[mi_row * mi_cols + mi_col];
            vp9_init_macroblockd(cm, xd, NULL);
            xd->mb_to_top_edge = -((mi_row * MI_SIZE) * 8);
            xd->mb_to_bottom_edge = ((cm->mi_rows - eb_vp9_num_8x8_blocks_high_lookup[bsize] - mi_row) * MI_SIZE) * 8;
            xd->mb_to_left_edge = -((mi_col * MI_SIZE) * 8);
            xd->mb_to_right_edge = ((cm->mi_cols - eb_vp9_num_8x8_blocks_wide_lookup[bsize] - mi_col) * MI_SIZE) * 8;
            xd->plane[0].subsampling_x = xd->plane[0].subsampling_y = 0;
            xd->plane[1].subsampling_x = xd->plane[1].subsampling_y = 1;
            xd->plane[2].subsampling_x = xd->plane[2].subsampling_y = 1;
            xd->lossless = 0;
            /* the block's coefficients and eobs the way the entropy coder hands them over: transform blocks in raster order of the
               block, each block's coefficients contiguous, eobs[] indexed in 4x4 units like the coefficients */
            int n_tb[3], tb_x4[3][256], tb_y4[3][256], tb_n[3][256];
            for (int p = 0; p < 3; p++) {
                const TX_SIZE ts = p ? get_uv_tx_size(m, &xd->plane[p]) : m->tx_size;
                const int     s = 1 << ts, bw4 = (eb_vp9_num_8x8_blocks_wide_lookup[bsize] * 2) >> (p ? 1 : 0), bh4 = (eb_vp9_num_8x8_blocks_high_lookup[bsize] * 2) >> (p ? 1 : 0);
                const int     x0 = (mi_col * 2) >> (p ? 1 : 0), y0 = (mi_row * 2) >> (p ? 1 : 0), pw4 = p ? w4 / 2 : w4;
                int           i = 0;
                n_tb[p] = 0;
                for (int y = 0; y < bh4; y += s)
                    for (int x = 0; x < bw4; x += s) {
                        const int e = emap[map_off[p] + (size_t)(y0 + y) * pw4 + x0 + x];
                        memcpy(blk_q[p] + i * 16, q + coeff_offset(p, x0 + x, y0 + y, sb_cols), sizeof(int16_t) * 16 * s * s);
                        blk_eob[p][i] = (uint16_t)e;
                        tb_x4[p][n_tb[p]] = x0 + x; tb_y4[p][n_tb[p]] = y0 + y; tb_n[p][n_tb[p]] = e + (e < 16 * s * s);
                        n_tb[p]++;
                        i += s * s;
                    }
                cpi->td.mb.plane[p].qcoeff = blk_q[p];
                cpi->td.mb.plane[p].eobs = blk_eob[p];
            }
            set_skip_context(xd, mi_row, mi_col);
            TOKENEXTRA  *t = tok;
            const double t0 = now();
            eb_vp9_tokenize_sb(cpi, xd, &cpi->td, &t, 0, 0, bsize);
            spent += now() - t0;
            if (m->skip) {
                if (t != tok) return 8;
                continue;
            }
            const TOKENEXTRA *rd = tok;
            for (int p = 0; p < 3; p++)
                for (int k = 0; k < n_tb[p]; k++) {
                    const int32_t h4r[4] = {p, tb_x4[p][k], tb_y4[p][k], tb_n[p][k]};
                    fwrite(h4r, 4, 4, out);
                    for (int j = 0; j < tb_n[p][k]; j++, rd++) {
                        const int     tkn = rd->token;
                        const int32_t rec[3] = {tkn, (tkn == ZERO_TOKEN || tkn == EOB_TOKEN) ? 0 : (int32_t)(uint16_t)rd->extra, (int32_t)((rd->context_tree - prob_base) / 3)};
                        fwrite(rec, 4, 3, out);
                    }
                    n_blocks++;
                }
            if (rd != t) return 9; /* the reference emitted another number of tokens than eob + (eob < n) per block */
        }
    }
    fwrite(cpi->td.rd_counts.coef_counts, sizeof(unsigned int), 4 * 2 * 2 * 6 * 6 * 12, out);
    fwrite(&spent, sizeof spent, 1, out);
    fseek(out, 0, SEEK_SET);
    fwrite(&n_blocks, 4, 1, out);
    fclose(out);
    return 0;
}
