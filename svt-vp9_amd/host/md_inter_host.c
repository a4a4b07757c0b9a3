/*
 * md_inter_host.c -- the host form of inter mode labelling (csrc/md_inter.hip): svt_hip_md_inter_modes_picture, the same inline text
 * the kernels call (csrc/md_inter_core.h over csrc/mvrefs_core.h) in the same two passes over a window built per SB in a local array:
 * labels into a scratch grid, then the MV-reference derivation over it.
 */
#include <stdlib.h>
#include <string.h>
#include "../../include/svtvp9_hip.h"
#include "../csrc/md_inter_core.h"

static void bad_grid(const svt_md_inter_picture *pic) {
    for (int k = 0; k < 4; k++) pic->d_status[k] = SVT_MODES_BAD_GRID;
}

int32_t svt_hip_md_inter_modes_picture(const svt_md_inter_picture *pic, int32_t width, int32_t height, int32_t mi_stride) {
    svt_tok_geom g;
    int          sb_cols, n_sb;
    if (!pic || !pic->d_lf_mi || !pic->d_mc_mi || !pic->d_ext_out || !pic->d_status || svt_tok_geom_of(width, height, mi_stride, &g, &sb_cols, &n_sb) ||
        (pic->ref_mask & 0xF1))
        return SVT_HIP_ERR_BAD_PARAMETER;
    const svt_mdi_frame m = svt_mdi_frame_of(pic);
    if (svt_mii_bad_frame(&m.f)) return SVT_HIP_ERR_BAD_PARAMETER;
    if (m.bad) {
        bad_grid(pic);
        return SVT_HIP_OK;
    }
    svt_mi_inter_ext *label = (svt_mi_inter_ext *)calloc((size_t)g.mi_rows * (size_t)mi_stride, sizeof *label);
    if (!label) return SVT_HIP_ERR_NO_RESOURCES;
    const svt_mvr_view v = svt_mvr_view_of(pic->d_lf_mi, pic->d_mc_mi, label, pic->ref_mask, pic->restrict_ref_mvs, pic->ref_frame_sign_bias);
    uint32_t inter_leaves = 0, new_leaves = 0, unfaithful_leaves = 0;
    for (int pass = 0; pass < 2; pass++) {
        if (pass)
            for (int r = 0; r < g.mi_rows; r++)
                for (int c = 0; c < g.mi_cols; c++)
                    if (svt_mvr_check(&v, &g, r, c) || svt_mdi_check(&v, &m, &g, r, c)) {
                        bad_grid(pic);
                        free(label);
                        return SVT_HIP_OK;
                    }
        for (int sb = 0; sb < n_sb; sb++) {
            const int sb_r = (sb / sb_cols) * 8, sb_c = (sb % sb_cols) * 8;
            uint32_t  win[SVT_MVR_WIN_WORDS];
            for (int i = 0; i < SVT_MVR_WIN * SVT_MVR_WIN; i++) {
                int           r, c;
                svt_mvr_entry e = svt_mvr_no_entry();
                if (svt_mvr_window_unit(&g, sb_r, sb_c, i, &r, &c)) e = pass ? svt_mvr_pack(&v, &g, r, c) : svt_mdi_pack(&v, &m, &g, r, c);
                svt_mvr_window_put(win, i, e);
            }
            for (int z = 0; z < 64; z++) {
                int ur, uc;
                svt_tok_unit_of(z, &ur, &uc);
                const int r = sb_r + ur, c = sb_c + uc;
                if (r >= g.mi_rows || c >= g.mi_cols) continue;
                const size_t idx = (size_t)r * (size_t)mi_stride + (size_t)c;
                if (!pass) {
                    const uint32_t w = svt_mdi_label_unit(&v, &m, &g, win, ur + 3, uc + 3, r, c); /* (little-endian word) */
                    memcpy((uint8_t *)(label + idx) + 8, &w, sizeof w);
                    continue;
                }
                const svt_mvr_unit_out o = svt_mvr_unit(&v, &g, win, ur + 3, uc + 3, r, c);
                int                    newmv, unfaithful;
                svt_mdi_count(&v, &m, &g, r, c, &o, &newmv, &unfaithful);
                inter_leaves += (uint32_t)o.inter_leaf;
                new_leaves += (uint32_t)newmv;
                unfaithful_leaves += (uint32_t)unfaithful;
                const uint32_t ext[3] = {o.e0, o.e1, o.e2}, cand[8] = {o.k0, o.k1, o.k2, o.k3, o.k4, o.k5, o.k6, o.k7};
                memcpy(pic->d_ext_out + idx, ext, sizeof ext);
                if (pic->d_cand) memcpy(pic->d_cand + idx, cand, sizeof cand);
            }
        }
    }
    free(label);
    pic->d_status[0] = inter_leaves;
    pic->d_status[1] = new_leaves;
    pic->d_status[2] = unfaithful_leaves;
    pic->d_status[3] = 0;
    return SVT_HIP_OK;
}
