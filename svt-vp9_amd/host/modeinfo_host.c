/*
 * modeinfo_host.c -- host-side (plain C) companions of the key-frame mode-info stage (csrc/modeinfo.hip):
 *   - svt_hip_modes_kf_picture, the host form (the same inline text the kernels call, csrc/modeinfo_core.h), which is what the CPU tests
 *     pin against the reference's write_partition / write_mb_modes_kf (VPX/vp9_bitstream.c:323-417);
 *   - the length of the segment list and the capacity of the bool buffer, which are host values.
 */
#include <string.h>
#include "../../include/svtvp9_hip.h"
#include "../csrc/modeinfo_core.h"

uint32_t svt_hip_modes_segments(int32_t width, int32_t height) {
    svt_tok_geom g;
    int          sb_cols, n_sb;
    return svt_tok_geom_of(width, height, width >> 3, &g, &sb_cols, &n_sb) ? 0 : (uint32_t)n_sb * 64u * 4u;
}
uint32_t svt_hip_modes_bools_capacity(int32_t width, int32_t height) {
    svt_tok_geom g;
    int          sb_cols, n_sb;
    return svt_tok_geom_of(width, height, width >> 3, &g, &sb_cols, &n_sb) ? 0 : (uint32_t)(g.mi_cols * g.mi_rows) * SVT_MI_UNIT_BOOLS;
}

int32_t svt_hip_modes_kf_picture(const svt_modes_tables *tables, const svt_modes_picture *pic, int32_t width, int32_t height, int32_t mi_stride) {
    svt_tok_geom g;
    int          sb_cols, n_sb;
    if (!tables || !pic || !pic->d_lf_mi || !pic->d_eob_map || !pic->d_tok_off || !pic->d_segments || !pic->d_n_bools || (!pic->d_bools && pic->capacity) ||
        svt_tok_geom_of(width, height, mi_stride, &g, &sb_cols, &n_sb))
        return SVT_HIP_ERR_BAD_PARAMETER;
    memset(pic->d_segments, 0, sizeof(svt_bool_segment) * 256 * (size_t)n_sb);
    for (int r = 0; r < g.mi_rows; r++)
        for (int c = 0; c < g.mi_cols; c++)
            if (svt_mi_check(pic->d_lf_mi, &g, r, c)) {
                *pic->d_n_bools = SVT_MODES_BAD_GRID;
                return SVT_HIP_OK;
            }
    uint64_t pos = 0;
    for (int sb = 0; sb < n_sb; sb++)
        for (int z = 0; z < 64; z++) {
            int ur, uc;
            svt_tok_unit_of(z, &ur, &uc);
            const int r = (sb / sb_cols) * 8 + ur, c = (sb % sb_cols) * 8 + uc;
            if (r >= g.mi_rows || c >= g.mi_cols) continue;
            uint16_t  rec[SVT_MI_UNIT_BOOLS + 64];
            const int n = svt_mi_unit_bools(pic->d_lf_mi, &g, r, c, tables, rec);
            if (n > SVT_MI_UNIT_BOOLS || n != svt_mi_unit_bools(pic->d_lf_mi, &g, r, c, NULL, NULL)) return SVT_HIP_ERR_BAD_PARAMETER; /* (the bound the capacity rests on) */
            if (!n) continue;
            svt_bool_segment *s = pic->d_segments + 4 * ((size_t)sb * 64 + z);
            uint32_t          first[3], count[3];
            svt_mi_leaf_tokens(pic->d_lf_mi, pic->d_eob_map, pic->d_tok_off, &g, r, c, first, count);
            s[0].first = (uint32_t)pos; s[0].count = (uint32_t)n; s[0].kind = 1;
            for (int p = 0; p < 3; p++)
                if (count[p]) { s[1 + p].first = first[p]; s[1 + p].count = count[p]; }
            for (int i = 0; i < n; i++)
                if (pos + i < pic->capacity) pic->d_bools[pos + i] = rec[i];
            pos += n;
        }
    *pic->d_n_bools = (uint32_t)pos;
    return SVT_HIP_OK;
}
