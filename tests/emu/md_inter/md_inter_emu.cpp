/*
 * md_inter_emu.cpp -- csrc/md_inter.hip on the CPU against svt_hip_md_inter_modes_picture (window_emu.h).  The 16 parameter bytes of a
 * picture: list_ref_frame[2], ref_frame_sign_bias[4], restrict_ref_mvs, allow_hp, reference_mode, comp_fixed_ref, comp_var_ref[2],
 * ref_mask, d_cand wanted, two unused; its grids: the two of svt_md_inter_picture.
 */
#include "md_inter.hip"
#include "window_emu.h"
struct md_inter_emu {
    typedef svt_md_inter_picture picture;
    enum { PAR = 16, EXT_GRID = 0, STATUS_WORDS = 4 };
    static picture desc(const uint8_t *par, const svt_lf_mode_info *mi, const svt_mc_mode_info *mc, const svt_mi_inter_ext *, svt_mi_inter_ext *ext_out,
                        svt_mvref_cand *cand, uint32_t *status) {
        picture d;
        memset(&d, 0, sizeof d);
        d.d_lf_mi = mi; d.d_mc_mi = mc; d.d_status = status;
        d.d_ext_out = ext_out; d.d_cand = par[13] ? cand : nullptr;
        memcpy(d.list_ref_frame, par, 2); memcpy(d.ref_frame_sign_bias, par + 2, 4);
        d.restrict_ref_mvs = par[6]; d.allow_hp = par[7]; d.reference_mode = par[8]; d.comp_fixed_ref = par[9];
        memcpy(d.comp_var_ref, par + 10, 2);
        d.ref_mask = par[12];
        return d;
    }
    static int device(svt_hip_ctx *ctx, int n, const picture *pics, int W, int H, int stride) { return svt_hip_md_inter_modes_batch_device(ctx, n, pics, W, H, stride); }
    static int host(const picture *pic, int W, int H, int stride) { return svt_hip_md_inter_modes_picture(pic, W, H, stride); }
};
int main(int argc, char **argv) { return window_emu_main<md_inter_emu>(argc, argv); }
