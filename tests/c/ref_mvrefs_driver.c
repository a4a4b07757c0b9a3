/*
 * ref_mvrefs_driver.c -- runs the REFERENCE's eb_vp9_find_mv_refs (VPX/vp9_mvref_common.c) for every leaf of 8x8 or larger and every
 * reference frame of a picture and writes what it returned: the two candidates, the return value and the mode context.  The grid is set
 * up the way the encode pass holds it: one ModeInfo per block, every unit's entry of mode_info_array pointing at it; per leaf the
 * EncDecContext's mi_row / mi_col / ep_block_stats_ptr->bsize and the four edges of xd as Codec/EbEncDecProcess.c:2055-2062 sets them;
 * cm's mi_rows, ref_frame_sign_bias and use_prev_frame_mvs; one tile.  Compiled by tests/gen_golden_mvrefs.py against the reference's
 * headers; the translation unit is compiled into this one by the include below.  Nothing of the reference is copied here.
 *
 * request : int32 magic, n_pics; per picture int32 width, height, restrict, sign_bias[4]; mi_rows * mi_cols records {uint8 sb_type,
 *           tx_size, skip, is_inter, filter_level, pad[3]}; as many {int16 mv_row[2], mv_col[2]; int8 ref_list[2]; uint8 bw8, bh8}; as many
 *           {int16 ref_mv_row[2], ref_mv_col[2]; uint8 ref_frame[2], mode, mode_context}
 * response: per picture mi_rows * mi_cols records {int16 mv_row[3][2], mv_col[3][2]; uint8 count[3], mode_context, pad[4]} -- filled at
 *           the origin of every leaf of 8x8 or larger, elsewhere 0 with counts 0xFF --, then double seconds of one pass over the picture
 *           (the best of REPEAT)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <time.h>

#include "vpx_dsp_rtcd.h"
#include "vp9_rtcd.h"
#include "vp9_mvref_common.c"

#define REPEAT 20

typedef struct { int16_t mv_row[2], mv_col[2]; int8_t ref_list[2]; uint8_t bw8, bh8; } mc_rec;
typedef struct { int16_t ref_mv_row[2], ref_mv_col[2]; uint8_t ref_frame[2], mode, mode_context; } ext_rec;
typedef struct { int16_t mv_row[3][2], mv_col[3][2]; uint8_t count[3], mode_context, pad[4]; } cand_rec;

static double drv_now(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[2];
    if (fread(hdr, 4, 2, f) != 2 || hdr[0] != 0x5246564d) return 4;
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 5;
    if (sizeof(mc_rec) != 12 || sizeof(ext_rec) != 12 || sizeof(cand_rec) != 32) return 6;

    EncDecContext *ctx = calloc(1, sizeof *ctx);
    VP9_COMMON    *cm = calloc(1, sizeof *cm);
    MACROBLOCKD   *xd = calloc(1, sizeof *xd);
    EpBlockStats   stats;
    memset(&stats, 0, sizeof stats);
    ctx->ep_block_stats_ptr = &stats;

    for (int k = 0; k < hdr[1]; k++) {
        int32_t p[7];
        if (fread(p, 4, 7, f) != 7 || p[0] < 8 || p[1] < 8 || (p[0] & 7) || (p[1] & 7)) return 8;
        const int mi_rows = p[1] >> 3, mi_cols = p[0] >> 3, units = mi_rows * mi_cols;
        uint8_t  *grid = malloc((size_t)units * 8);
        mc_rec   *mc = malloc(sizeof *mc * (size_t)units);
        ext_rec  *er = malloc(sizeof *er * (size_t)units);
        cand_rec *res = calloc((size_t)units, sizeof *res);
        if (fread(grid, 8, (size_t)units, f) != (size_t)units || fread(mc, 12, (size_t)units, f) != (size_t)units || fread(er, 12, (size_t)units, f) != (size_t)units) return 9;
        cm->mi_rows = mi_rows; cm->mi_cols = mi_cols; cm->mi_stride = mi_cols;
        cm->use_prev_frame_mvs = p[2] ? EB_TRUE : EB_FALSE;
        for (int i = 0; i < 4; i++) cm->ref_frame_sign_bias[i] = p[3 + i];
        xd->tile.mi_row_start = 0; xd->tile.mi_row_end = mi_rows; xd->tile.mi_col_start = 0; xd->tile.mi_col_end = mi_cols;
        ModeInfo  *blocks = calloc((size_t)units, sizeof *blocks);
        ModeInfo **vis = calloc((size_t)units, sizeof *vis);
        ctx->mode_info_array = vis;
        ctx->mi_stride = mi_cols;
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
                    m->mode = (PREDICTION_MODE)(g[0] < BLOCK_8X8 ? g[5] >> 4 : g[6]); /* (four 4x4 blocks: the last one's, Codec/EbEncDecProcess.c:2208-2212) */
                    continue;
                }
                m->ref_frame[0] = (MV_REFERENCE_FRAME)er[u].ref_frame[0];
                m->ref_frame[1] = er[u].ref_frame[1] ? (MV_REFERENCE_FRAME)er[u].ref_frame[1] : NONE;
                m->mode = (PREDICTION_MODE)er[u].mode;
                for (int ref = 0; ref < 2; ref++) { m->mv[ref].as_mv.row = mc[u].mv_row[ref]; m->mv[ref].as_mv.col = mc[u].mv_col[ref]; }
            }
        double best = 1e30;
        for (int rep = 0; rep < REPEAT; rep++) {
            const double t0 = drv_now();
            for (int r = 0; r < mi_rows; r++)
                for (int c = 0; c < mi_cols; c++) {
                    const int       u = r * mi_cols + c;
                    const ModeInfo *m = vis[u];
                    cand_rec       *o = &res[u];
                    memset(o, 0, sizeof *o);
                    o->count[0] = o->count[1] = o->count[2] = 0xFF;
                    if (m != &blocks[u] || m->sb_type < BLOCK_8X8) continue;
                    stats.bsize = m->sb_type;
                    ctx->mi_row = r; ctx->mi_col = c;
                    xd->mb_to_top_edge = -((r * MI_SIZE) * 8);
                    xd->mb_to_bottom_edge = ((cm->mi_rows - eb_vp9_num_8x8_blocks_high_lookup[m->sb_type] - r) * MI_SIZE) * 8;
                    xd->mb_to_left_edge = -((c * MI_SIZE) * 8);
                    xd->mb_to_right_edge = ((cm->mi_cols - eb_vp9_num_8x8_blocks_wide_lookup[m->sb_type] - c) * MI_SIZE) * 8;
                    uint8_t mode_context[MAX_REF_FRAMES] = {0};
                    for (int ref = LAST_FRAME; ref <= ALTREF_FRAME; ref++) {
                        int_mv    list[MAX_MV_REF_CANDIDATES];
                        const int n = eb_vp9_find_mv_refs(ctx, cm, xd, (ModeInfo *)NULL, (MV_REFERENCE_FRAME)ref, list, r, c, mode_context);
                        for (int i = 0; i < 2; i++) { o->mv_row[ref - 1][i] = list[i].as_mv.row; o->mv_col[ref - 1][i] = list[i].as_mv.col; }
                        o->count[ref - 1] = (uint8_t)n;
                    }
                    if (mode_context[LAST_FRAME] != mode_context[GOLDEN_FRAME] || mode_context[LAST_FRAME] != mode_context[ALTREF_FRAME]) return 10;
                    o->mode_context = mode_context[LAST_FRAME];
                }
            const double dt = drv_now() - t0;
            best = dt < best ? dt : best;
        }
        fwrite(res, sizeof *res, (size_t)units, out);
        fwrite(&best, 8, 1, out);
        free(grid); free(mc); free(er); free(res); free(blocks); free(vis);
    }
    fclose(f);
    fclose(out);
    return 0;
}
