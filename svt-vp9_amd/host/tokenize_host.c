/*
 * tokenize_host.c -- host-side (plain C) companions of the coefficient tokeniser (csrc/tokenize.hip):
 *   - the scan orders in the layout svt_rate_block.scan_off addresses, built at first use from the committed inverse scans
 *     (host/vp9_tables.inc through svt_hip_vp9_iscan_tables) and the neighbour rule of csrc/tokenize_core.h: no second table file;
 *   - svt_hip_tokenize_picture, the host form of the picture-level tokeniser (the same inline text the kernels call), which is what
 *     the CPU tests pin against the reference's eb_vp9_tokenize_sb (VPX/vp9_tokenize.c:397-430).
 */
#include <pthread.h>
#include <string.h>
#include "../../include/svtvp9_hip.h"
#include "../csrc/tokenize_core.h"

#define TOK_SCAN_ENTRIES (4 * (50 + 194 + 770 + 3074))

static int16_t        g_scan[TOK_SCAN_ENTRIES];
static uint32_t       g_scan_off[16];
static pthread_once_t g_scan_once = PTHREAD_ONCE_INIT;

static void build_scan_tables(void) {
    const uint32_t *ioff = NULL;
    const int16_t  *iscan = svt_hip_vp9_iscan_tables(&ioff, NULL);
    memset(g_scan, 0, sizeof g_scan); /* position 0 and the trailing pair are (0, 0) */
    for (int ts = 0; ts < 4; ts++)
        for (int tt = 0; tt < 4; tt++) {
            const int n = 16 << (2 * ts), off = svt_tok_scan_offset(ts, tt);
            int16_t  *scan = g_scan + off, *nb = scan + n;
            g_scan_off[ts * 4 + tt] = (uint32_t)off;
            for (int p = 0; p < n; p++) scan[iscan[ioff[ts * 4 + tt] + p]] = (int16_t)p;
            for (int c = 1; c < n; c++) {
                int a, b;
                svt_tok_neighbors(ts, tt, scan[c], &a, &b);
                nb[2 * c] = (int16_t)a; nb[2 * c + 1] = (int16_t)b;
            }
        }
}

const int16_t *svt_hip_vp9_scan_tables(const uint32_t **offsets16, int32_t *entries) {
    pthread_once(&g_scan_once, build_scan_tables);
    if (offsets16) *offsets16 = g_scan_off;
    if (entries) *entries = TOK_SCAN_ENTRIES;
    return g_scan;
}

uint32_t svt_hip_tokenize_capacity(int32_t width, int32_t height) {
    if (width < 8 || height < 8) return 0;
    const uint64_t px = (uint64_t)width * (uint64_t)height, cap = px * 3 / 2 + px * 3 / 32;
    return cap > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cap;
}

int32_t svt_hip_tokenize_blocks_host(const int16_t *qcoeff, size_t coeff_count, const svt_rate_block *blocks, int32_t n_blocks, uint32_t *tokens,
                                     uint32_t capacity, uint32_t *tok_off, uint32_t *counts) {
    if (!qcoeff || !blocks || n_blocks < 1 || !tok_off || (!tokens && capacity)) return SVT_HIP_ERR_BAD_PARAMETER;
    const int16_t *scan_all = svt_hip_vp9_scan_tables(NULL, NULL);
    if (counts) memset(counts, 0, SVT_TOK_COUNTS * sizeof(uint32_t));
    uint64_t pos = 0;
    for (int i = 0; i < n_blocks; i++) {
        const svt_rate_block *b = &blocks[i];
        if (b->tx_size > 3 || b->plane_type > 1 || b->is_inter > 1 || b->ctx > 2) return SVT_HIP_ERR_BAD_PARAMETER;
        const size_t   n = (size_t)16 << (2 * b->tx_size);
        const uint32_t first = (uint32_t)svt_tok_scan_offset(b->tx_size, 0), tt = (b->scan_off - first) / (uint32_t)(3 * n + 2);
        if (b->eob > n || b->coeff_off + n > coeff_count || b->scan_off < first || b->scan_off != first + tt * (3 * n + 2) || tt > 3) return SVT_HIP_ERR_BAD_PARAMETER;
        const int cnt = b->eob + (b->eob < n);
        tok_off[i] = (uint32_t)pos;
        for (int c = 0; c < cnt; c++) {
            const uint32_t rec = svt_tok_position(qcoeff + b->coeff_off, scan_all + b->scan_off, c, b->eob, b->tx_size, (int)tt, b->plane_type, b->is_inter, b->ctx);
            if (pos + c < capacity) tokens[pos + c] = rec;
            if (counts) counts[SVT_TOK_PROB_ROW(rec) * 12 + SVT_TOK_TOKEN(rec)]++;
        }
        pos += cnt;
    }
    tok_off[n_blocks] = (uint32_t)pos;
    return SVT_HIP_OK;
}

int32_t svt_hip_tokenize_picture(const svt_tok_picture *pic, int32_t width, int32_t height, int32_t mi_stride) {
    if (!pic || !pic->d_lf_mi || !pic->d_qcoeff || !pic->d_eob_map || !pic->d_tok_off || !pic->d_sb_off || (!pic->d_tokens && pic->capacity) || width < 8 ||
        height < 8 || (width & 7) || (height & 7) || mi_stride < (width >> 3))
        return SVT_HIP_ERR_BAD_PARAMETER;
    const int16_t     *scan_all = svt_hip_vp9_scan_tables(NULL, NULL);
    const svt_tok_geom g = {mi_stride, height >> 3, width >> 3, width >> 2, height >> 2};
    const int          sb_cols = (width + 63) >> 6, sb_rows = (height + 63) >> 6;
    const size_t       map_n = (size_t)g.w4 * g.h4 * 3 / 2;
    for (size_t i = 0; i < map_n; i++) pic->d_tok_off[i] = SVT_TOK_NONE;
    if (pic->d_counts) memset(pic->d_counts, 0, SVT_TOK_COUNTS * sizeof(uint32_t));
    uint64_t pos = 0;
    for (int sb = 0; sb < sb_rows * sb_cols; sb++) {
        const int sr = sb / sb_cols, sc = sb % sb_cols;
        pic->d_sb_off[sb] = (uint32_t)pos;
        for (int plane = 0; plane < 3; plane++) {
            const int pw4 = plane ? g.w4 >> 1 : g.w4, units = plane ? 64 : 256, side = plane ? 8 : 16;
            for (int z = 0; z < units; z++) { /* 4x4 units of the SB's plane area in z-order */
                int lx = 0, ly = 0;
                for (int bit = 0; bit < 4; bit++) { lx |= ((z >> (2 * bit)) & 1) << bit; ly |= ((z >> (2 * bit + 1)) & 1) << bit; }
                const int     x4 = sc * side + lx, y4 = sr * side + ly;
                svt_tok_block k;
                if (!svt_tok_block_at(pic->d_lf_mi, pic->d_eob_map, &g, plane, x4, y4, &k)) continue;
                const int16_t *q = pic->d_qcoeff + (size_t)sb * SVT_SB_COEFFS + (plane == 0 ? 0 : plane == 1 ? 4096 : 5120) + z * 16;
                const int16_t *scan = scan_all + svt_tok_scan_offset(k.ts, k.tt);
                const int      cnt = svt_tok_count(&k);
                pic->d_tok_off[svt_tok_map_offset(&g, plane) + y4 * pw4 + x4] = (uint32_t)pos;
                for (int c = 0; c < cnt; c++) {
                    const uint32_t rec = svt_tok_position(q, scan, c, k.eob, k.ts, k.tt, plane != 0, k.inter, k.ctx);
                    if (pos + c < pic->capacity) pic->d_tokens[pos + c] = rec;
                    if (pic->d_counts) pic->d_counts[SVT_TOK_PROB_ROW(rec) * 12 + SVT_TOK_TOKEN(rec)]++;
                }
                pos += cnt;
            }
        }
    }
    pic->d_sb_off[sb_rows * sb_cols] = (uint32_t)pos;
    return SVT_HIP_OK;
}
