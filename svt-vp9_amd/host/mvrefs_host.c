/*
 * mvrefs_host.c -- the host form of the MV-reference derivation (csrc/mvrefs.hip): svt_hip_mvrefs_picture, the same inline text the
 * kernels call (csrc/mvrefs_core.h) over a window built per SB in a local array, which is what the CPU tests pin against the reference's
 * eb_vp9_find_mv_refs (VPX/vp9_mvref_common.c:20-197).
 */
#include <string.h>
#include "../../include/svtvp9_hip.h"
#include "../csrc/mvrefs_core.h"

int32_t svt_hip_mvrefs_picture(const svt_mvrefs_picture *pic, int32_t width, int32_t height, int32_t mi_stride) {
    svt_tok_geom g;
    int          sb_cols, n_sb;
    if (!pic || !pic->d_lf_mi || !pic->d_mc_mi || !pic->d_ext || !pic->d_status || svt_tok_geom_of(width, height, mi_stride, &g, &sb_cols, &n_sb) ||
        (pic->ref_mask & 0xF1) || pic->d_ext_out == pic->d_ext)
        return SVT_HIP_ERR_BAD_PARAMETER;
    const svt_mvr_view v = svt_mvr_view_of(pic->d_lf_mi, pic->d_mc_mi, pic->d_ext, pic->ref_mask, pic->restrict_ref_mvs, pic->ref_frame_sign_bias);
    for (int r = 0; r < g.mi_rows; r++)
        for (int c = 0; c < g.mi_cols; c++)
            if (svt_mvr_check(&v, &g, r, c)) {
                pic->d_status[0] = pic->d_status[1] = SVT_MODES_BAD_GRID;
                return SVT_HIP_OK;
            }
    uint32_t contradicting = 0, inter_leaves = 0;
    for (int sb = 0; sb < n_sb; sb++) {
        const int sb_r = (sb / sb_cols) * 8, sb_c = (sb % sb_cols) * 8;
        uint32_t  win[SVT_MVR_WIN_WORDS];
        for (int i = 0; i < SVT_MVR_WIN * SVT_MVR_WIN; i++) {
            int           r, c;
            svt_mvr_entry e = svt_mvr_no_entry();
            if (svt_mvr_window_unit(&g, sb_r, sb_c, i, &r, &c)) e = svt_mvr_pack(&v, &g, r, c);
            svt_mvr_window_put(win, i, e);
        }
        for (int z = 0; z < 64; z++) {
            int ur, uc;
            svt_tok_unit_of(z, &ur, &uc);
            const int r = sb_r + ur, c = sb_c + uc;
            if (r >= g.mi_rows || c >= g.mi_cols) continue;
            const svt_mvr_unit_out o = svt_mvr_unit(&v, &g, win, ur + 3, uc + 3, r, c);
            const size_t           idx = (size_t)r * (size_t)mi_stride + (size_t)c;
            contradicting += (uint32_t)o.contradicts;
            inter_leaves += (uint32_t)o.inter_leaf;
            const uint32_t         ext[3] = {o.e0, o.e1, o.e2}, cand[8] = {o.k0, o.k1, o.k2, o.k3, o.k4, o.k5, o.k6, o.k7}; /* (little-endian words) */
            if (pic->d_ext_out) memcpy(pic->d_ext_out + idx, ext, sizeof ext);
            if (pic->d_cand) memcpy(pic->d_cand + idx, cand, sizeof cand);
        }
    }
    pic->d_status[0] = contradicting;
    pic->d_status[1] = inter_leaves;
    return SVT_HIP_OK;
}
