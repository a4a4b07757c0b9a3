/*
 * ref_md_inter_driver.c -- labels the inter leaves of a picture with the REFERENCE's eb_vp9_find_mv_refs (VPX/vp9_mvref_common.c): per
 * leaf of 8x8 or larger and per reference frame of the leaf the two candidates and the return value, then the four-way comparison in
 * plain C on the reference's int_mv values -- NEARESTMV if every MV is the first candidate and one was found, else NEARMV if every MV is
 * the second and two were found, else ZEROMV if every MV is zero, else NEWMV --, then, with every leaf's mode in place, eb_vp9_find_mv_refs
 * once more for mbmi_ext's ref_mvs[ref_frame][0] and mode_context.  The grid is set up as tests/c/ref_mvrefs_driver.c sets it up; the
 * reference frames come from the prediction grid's ref_list through list_ref_frame.  The tile bytes of the labelled pictures are written
 * by tests/c/ref_modes_inter_driver.c (write_partition, pack_inter_mode_mvs, pack_mb_tokens), which tests/gen_golden_md_inter.py runs on
 * this driver's records.  Compiled by that generator against the reference's headers; the translation unit is compiled into this one by
 * the include below.  Nothing of the reference is copied here.
 *
 * request : int32 magic, n_pics; per picture int32 width, height, restrict, sign_bias[4], list_ref_frame[2]; mi_rows * mi_cols records
 *           {uint8 sb_type, tx_size, skip, is_inter, filter_level, pad[3]}; as many {int16 mv_row[2], mv_col[2]; int8 ref_list[2]; uint8 bw8, bh8}
 * response: per picture mi_rows * mi_cols records {int16 ref_mv_row[2], ref_mv_col[2]; uint8 ref_frame[2], mode, mode_context}: ref_frame
 *           at every unit, the other fields at the origin of an inter leaf, everything else 0
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

#include "vpx_dsp_rtcd.h"
#include "vp9_rtcd.h"
#include "vp9_mvref_common.c"

typedef struct { int16_t mv_row[2], mv_col[2]; int8_t ref_list[2]; uint8_t bw8, bh8; } mc_rec;
typedef struct { int16_t ref_mv_row[2], ref_mv_col[2]; uint8_t ref_frame[2], mode, mode_context; } ext_rec;

static void at_leaf(EncDecContext *ctx, VP9_COMMON *cm, MACROBLOCKD *xd, EpBlockStats *stats, const ModeInfo *m, int r, int c) {
    stats->bsize = m->sb_type;
    ctx->mi_row = r; ctx->mi_col = c;
    xd->mb_to_top_edge = -((r * MI_SIZE) * 8);
    xd->mb_to_bottom_edge = ((cm->mi_rows - eb_vp9_num_8x8_blocks_high_lookup[m->sb_type] - r) * MI_SIZE) * 8;
    xd->mb_to_left_edge = -((c * MI_SIZE) * 8);
    xd->mb_to_right_edge = ((cm->mi_cols - eb_vp9_num_8x8_blocks_wide_lookup[m->sb_type] - c) * MI_SIZE) * 8;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[2];
    if (fread(hdr, 4, 2, f) != 2 || hdr[0] != 0x49444d4c) return 4;
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 5;
    if (sizeof(mc_rec) != 12 || sizeof(ext_rec) != 12) return 6;

    EncDecContext *ctx = calloc(1, sizeof *ctx);
    VP9_COMMON    *cm = calloc(1, sizeof *cm);
    MACROBLOCKD   *xd = calloc(1, sizeof *xd);
    EpBlockStats   stats;
    memset(&stats, 0, sizeof stats);
    ctx->ep_block_stats_ptr = &stats;

    for (int k = 0; k < hdr[1]; k++) {
        int32_t p[9];
        if (fread(p, 4, 9, f) != 9 || p[0] < 8 || p[1] < 8 || (p[0] & 7) || (p[1] & 7)) return 8;
        const int mi_rows = p[1] >> 3, mi_cols = p[0] >> 3, units = mi_rows * mi_cols;
        uint8_t *grid = malloc((size_t)units * 8);
        mc_rec  *mc = malloc(sizeof *mc * (size_t)units);
        ext_rec *res = calloc((size_t)units, sizeof *res);
        uint8_t *label = calloc((size_t)units, 1);
        if (fread(grid, 8, (size_t)units, f) != (size_t)units || fread(mc, 12, (size_t)units, f) != (size_t)units) return 9;
        cm->mi_rows = mi_rows; cm->mi_cols = mi_cols; cm->mi_stride = mi_cols;
        cm->use_prev_frame_mvs = p[2] ? EB_TRUE : EB_FALSE;
        for (int i = 0; i < 4; i++) cm->ref_frame_sign_bias[i] = p[3 + i];
        xd->tile.mi_row_start = 0; xd->tile.mi_row_end = mi_rows; xd->tile.mi_col_start = 0; xd->tile.mi_col_end = mi_cols;
        ModeInfo  *blocks = calloc((size_t)units, sizeof *blocks);
        ModeInfo **vis = calloc((size_t)units, sizeof *vis);
        ctx->mode_info_array = vis;
        ctx->mi_stride = mi_cols;
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
                    m->mode = (PREDICTION_MODE)(g[0] < BLOCK_8X8 ? g[5] >> 4 : g[6]);
                    continue;
                }
                if (mc[u].ref_list[0] < 0 || mc[u].ref_list[0] > 1 || mc[u].ref_list[1] > 1) return 10;
                m->ref_frame[0] = (MV_REFERENCE_FRAME)p[7 + mc[u].ref_list[0]];
                m->ref_frame[1] = mc[u].ref_list[1] < 0 ? NONE : (MV_REFERENCE_FRAME)p[7 + mc[u].ref_list[1]];
                m->mode = NEWMV; /* (a placeholder the first pass does not look at: it discards the mode context) */
                for (int ref = 0; ref < 2; ref++) { m->mv[ref].as_mv.row = mc[u].mv_row[ref]; m->mv[ref].as_mv.col = mc[u].mv_col[ref]; }
            }
        for (int pass = 0; pass < 2; pass++) {
            for (int r = 0; r < mi_rows; r++)
                for (int c = 0; c < mi_cols; c++) {
                    const int u = r * mi_cols + c;
                    ModeInfo *m = vis[u];
                    ext_rec  *o = &res[u];
                    if (pass) {
                        o->ref_frame[0] = m->ref_frame[0] > INTRA_FRAME ? (uint8_t)m->ref_frame[0] : 0;
                        o->ref_frame[1] = m->ref_frame[1] > INTRA_FRAME ? (uint8_t)m->ref_frame[1] : 0;
                    }
                    if (m != &blocks[u] || m->sb_type < BLOCK_8X8 || m->ref_frame[0] <= INTRA_FRAME) continue;
                    at_leaf(ctx, cm, xd, &stats, m, r, c);
                    const int n_ref = m->ref_frame[1] > INTRA_FRAME ? 2 : 1;
                    uint8_t   mode_context[MAX_REF_FRAMES] = {0};
                    int       nearest = 1, near = 1, zero = 1;
                    for (int i = 0; i < n_ref; i++) {
                        int_mv    list[MAX_MV_REF_CANDIDATES];
                        const int n = eb_vp9_find_mv_refs(ctx, cm, xd, (ModeInfo *)NULL, m->ref_frame[i], list, r, c, mode_context);
                        nearest &= n >= 1 && m->mv[i].as_int == list[0].as_int;
                        near &= n == 2 && m->mv[i].as_int == list[1].as_int;
                        zero &= m->mv[i].as_int == 0;
                        if (pass) { o->ref_mv_row[i] = list[0].as_mv.row; o->ref_mv_col[i] = list[0].as_mv.col; }
                    }
                    if (!pass) label[u] = nearest ? NEARESTMV : near ? NEARMV : zero ? ZEROMV : NEWMV;
                    else { o->mode = (uint8_t)m->mode; o->mode_context = mode_context[m->ref_frame[0]]; }
                }
            if (!pass)
                for (int u = 0; u < units; u++)
                    if (label[u]) blocks[u].mode = (PREDICTION_MODE)label[u];
        }
        fwrite(res, sizeof *res, (size_t)units, out);
        free(grid); free(mc); free(res); free(label); free(blocks); free(vis);
    }
    fclose(f);
    fclose(out);
    return 0;
}
