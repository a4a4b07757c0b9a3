/*
 * mvrefs_emu.cpp -- csrc/mvrefs.hip on the CPU against svt_hip_mvrefs_picture (window_emu.h).  The 8 parameter bytes of a picture:
 * ref_mask, restrict_ref_mvs, ref_frame_sign_bias[4], d_ext_out wanted, d_cand wanted; its grids: the three of svt_mvrefs_picture.
 */
#include "mvrefs.hip"
#include "window_emu.h"
struct mvrefs_emu {
    typedef svt_mvrefs_picture picture;
    enum { PAR = 8, EXT_GRID = 1, STATUS_WORDS = 2 };
    static picture desc(const uint8_t *par, const svt_lf_mode_info *mi, const svt_mc_mode_info *mc, const svt_mi_inter_ext *ext, svt_mi_inter_ext *ext_out,
                        svt_mvref_cand *cand, uint32_t *status) {
        picture d;
        memset(&d, 0, sizeof d);
        d.d_lf_mi = mi; d.d_mc_mi = mc; d.d_ext = ext; d.d_status = status;
        d.d_ext_out = par[6] ? ext_out : nullptr; d.d_cand = par[7] ? cand : nullptr;
        d.ref_mask = par[0]; d.restrict_ref_mvs = par[1];
        memcpy(d.ref_frame_sign_bias, par + 2, 4);
        return d;
    }
    static int device(svt_hip_ctx *ctx, int n, const picture *pics, int W, int H, int stride) { return svt_hip_mvrefs_batch_device(ctx, n, pics, W, H, stride); }
    static int host(const picture *pic, int W, int H, int stride) { return svt_hip_mvrefs_picture(pic, W, H, stride); }
};
int main(int argc, char **argv) { return window_emu_main<mvrefs_emu>(argc, argv); }
