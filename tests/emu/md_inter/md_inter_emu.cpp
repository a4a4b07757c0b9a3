/*
 * md_inter_emu.cpp -- csrc/md_inter.hip itself (kernels and entry point, included below) on the CPU through the stand-in runtime of
 * tests/emu/hip/hip_runtime.h, compared with svt_hip_md_inter_modes_picture: every byte of d_ext_out and d_cand with the guard bytes behind
 * them, and the four status words (the two buffers are left out of the comparison for a grid the stage does not take: their contents
 * are unspecified).  The grids are allocated to exactly mi_rows x mi_stride records.
 * argv[1]: a file holding int32 n_groups; per group int32 width, height, mi_stride, n_pics, then per picture 16 bytes
 * (list_ref_frame[2], ref_frame_sign_bias[4], restrict_ref_mvs, allow_hp, reference_mode, comp_fixed_ref, comp_var_ref[2], ref_mask,
 * d_cand wanted, two unused) and the two grids (svt_lf_mode_info, svt_mc_mode_info).  A group is one batch call.
 */
#include "md_inter.hip"
#include "emu_harness.h"
#define GUARD 64
struct pic_bufs {
    std::vector<svt_lf_mode_info> mi;
    std::vector<svt_mc_mode_info> mc;
    std::vector<uint32_t> ext_out[2], status[2]; /* (4-byte aligned, as the device's buffers are) */
    std::vector<uint4> cand[2];
    uint8_t par[16];
    svt_md_inter_picture desc(int k) {
        svt_md_inter_picture d;
        memset(&d, 0, sizeof d);
        d.d_lf_mi = mi.data(); d.d_mc_mi = mc.data();
        d.d_ext_out = (svt_mi_inter_ext *)ext_out[k].data(); d.d_cand = par[13] ? (svt_mvref_cand *)cand[k].data() : nullptr;
        d.d_status = status[k].data();
        memcpy(d.list_ref_frame, par, 2); memcpy(d.ref_frame_sign_bias, par + 2, 4);
        d.restrict_ref_mvs = par[6]; d.allow_hp = par[7]; d.reference_mode = par[8]; d.comp_fixed_ref = par[9];
        memcpy(d.comp_var_ref, par + 10, 2);
        d.ref_mask = par[12];
        return d;
    }
};
int main(int argc, char **argv) {
    static svt_hip_ctx ctx;
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    int32_t n_groups = 0;
    if (!f || fread(&n_groups, 4, 1, f) != 1) return 2;
    int bad = 0;
    for (int g = 0; g < n_groups; g++) {
        int32_t whn[4];
        if (fread(whn, 4, 4, f) != 4) return 3;
        const int W = whn[0], H = whn[1], stride = whn[2], n_pics = whn[3], units = stride * (H / 8);
        std::vector<pic_bufs> P(n_pics);
        std::vector<svt_md_inter_picture> d(n_pics);
        for (int i = 0; i < n_pics; i++) {
            pic_bufs &p = P[i];
            p.mi.resize(units); p.mc.resize(units);
            if (fread(p.par, 1, 16, f) != 16 || fread(p.mi.data(), 8, units, f) != (size_t)units || fread(p.mc.data(), 12, units, f) != (size_t)units) return 4;
            for (int k = 0; k < 2; k++) {
                p.ext_out[k].assign(3 * (size_t)units + GUARD, 0xA5A5A5A5u); p.status[k].assign(4 + GUARD, 0x77777777u);
                p.cand[k].assign(2 * (size_t)units + GUARD, make_uint4(0x5A5A5A5Au, 0x5A5A5A5Au, 0x5A5A5A5Au, 0x5A5A5A5Au));
            }
            d[i] = p.desc(0);
        }
        const int r1 = svt_hip_md_inter_modes_batch_device(&ctx, n_pics, d.data(), W, H, stride);
        for (int i = 0; i < n_pics; i++) {
            pic_bufs &p = P[i];
            svt_md_inter_picture h = p.desc(1);
            const int  r2 = svt_hip_md_inter_modes_picture(&h, W, H, stride);
            const bool taken = p.status[1][0] != SVT_MODES_BAD_GRID;
            bool       ok = !r1 && !r2 && p.status[0] == p.status[1];
            if (taken) ok = ok && p.ext_out[0] == p.ext_out[1] && !memcmp(p.cand[0].data(), p.cand[1].data(), sizeof(uint4) * p.cand[0].size());
            for (int k = 0; k < GUARD; k++) ok = ok && p.ext_out[0][3 * (size_t)units + k] == 0xA5A5A5A5u && p.cand[0][2 * (size_t)units + k].x == 0x5A5A5A5Au;
            printf("group %d %dx%d stride %d picture %d status %u/%u %u/%u %u/%u %u/%u %s\n", g, W, H, stride, i, p.status[0][0], p.status[1][0], p.status[0][1],
                   p.status[1][1], p.status[0][2], p.status[1][2], p.status[0][3], p.status[1][3], ok ? "ok" : "MISMATCH");
            bad += !ok;
        }
    }
    printf("bad %d\n", bad);
    return bad;
}
