/*
 * modeinfo_inter_emu.cpp -- csrc/modeinfo_inter.hip itself (kernels and entry points, included below) on the CPU through the stand-in
 * runtime of tests/emu/hip/hip_runtime.h, compared with svt_hip_modes_inter_picture: bool records up to the capacity, the guard words behind
 * them, every segment record, the bool total.  argv[1]: a file holding one svt_modes_inter_tables, then int32 n_groups; per group int32
 * width, height, mi_stride, n_pics, then per picture int32 capacity, 9 bytes of frame parameters (reference_mode, allow_hp,
 * comp_fixed_ref, comp_var_ref[2], ref_frame_sign_bias[4]), the three grids (mi_rows x mi_stride records each: svt_lf_mode_info,
 * svt_mc_mode_info, svt_mi_inter_ext), the eob map (uint16), the tokeniser's offsets (uint32).  A group is one batch call.
 */
#include "modeinfo_inter.hip"
#include "emu_harness.h"
struct pic_bufs {
    std::vector<svt_lf_mode_info> mi;
    std::vector<svt_mc_mode_info> mc;
    std::vector<svt_mi_inter_ext> ext;
    std::vector<uint16_t> emap, bools[2];
    std::vector<uint32_t> tok_off, n[2];
    std::vector<uint4> segs[2]; /* (16-byte aligned by the allocator's alignment of uint4) */
    uint32_t cap;
    uint8_t  frame[9];
    svt_modes_inter_picture desc(int k) {
        svt_modes_inter_picture d;
        memset(&d, 0, sizeof d);
        d.d_lf_mi = mi.data(); d.d_mc_mi = mc.data(); d.d_ext = ext.data(); d.d_eob_map = emap.data(); d.d_tok_off = tok_off.data();
        d.d_bools = bools[k].data(); d.d_segments = (svt_bool_segment *)segs[k].data(); d.d_n_bools = n[k].data(); d.capacity = cap;
        d.reference_mode = frame[0]; d.allow_hp = frame[1]; d.comp_fixed_ref = frame[2]; d.comp_var_ref[0] = frame[3]; d.comp_var_ref[1] = frame[4];
        memcpy(d.ref_frame_sign_bias, frame + 5, 4);
        return d;
    }
};
int main(int argc, char **argv) {
    static svt_hip_ctx ctx;
    svt_modes_inter_tables tab;
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    int32_t n_groups = 0;
    if (!f || fread(&tab, sizeof tab, 1, f) != 1 || fread(&n_groups, 4, 1, f) != 1) return 2;
    svt_hip_modes_inter_set_tables(&ctx, &tab);
    int bad = 0;
    for (int g = 0; g < n_groups; g++) {
        int32_t whn[4];
        if (fread(whn, 4, 4, f) != 4) return 3;
        const int W = whn[0], H = whn[1], stride = whn[2], n_pics = whn[3], units = stride * (H / 8), map_n = (W / 4) * (H / 4) * 3 / 2;
        const uint32_t n_seg = svt_hip_modes_segments(W, H);
        std::vector<pic_bufs> P(n_pics);
        std::vector<svt_modes_inter_picture> d(n_pics);
        for (int i = 0; i < n_pics; i++) {
            int32_t cap;
            pic_bufs &p = P[i];
            p.mi.resize(units); p.mc.resize(units); p.ext.resize(units); p.emap.resize(map_n); p.tok_off.resize(map_n);
            if (fread(&cap, 4, 1, f) != 1 || fread(p.frame, 1, 9, f) != 9 || fread(p.mi.data(), 8, units, f) != (size_t)units ||
                fread(p.mc.data(), 12, units, f) != (size_t)units || fread(p.ext.data(), 12, units, f) != (size_t)units ||
                fread(p.emap.data(), 2, map_n, f) != (size_t)map_n || fread(p.tok_off.data(), 4, map_n, f) != (size_t)map_n)
                return 4;
            p.cap = (uint32_t)cap;
            for (int k = 0; k < 2; k++) {
                p.bools[k].assign(p.cap + 64, 0xA5A5); p.n[k].assign(4, 0x77777777u);
                p.segs[k].assign(n_seg * 3 / 4 + 8, make_uint4(0x5A5A5A5Au, 0x5A5A5A5Au, 0x5A5A5A5Au, 0x5A5A5A5Au));
            }
            d[i] = p.desc(0);
        }
        const int r1 = svt_hip_modes_inter_batch_device(&ctx, n_pics, d.data(), W, H, stride);
        for (int i = 0; i < n_pics; i++) {
            pic_bufs &p = P[i];
            svt_modes_inter_picture h = p.desc(1);
            const int  r2 = svt_hip_modes_inter_picture(&tab, &h, W, H, stride);
            const bool ok = !r1 && !r2 && p.n[0] == p.n[1] && p.bools[0] == p.bools[1] && !memcmp(p.segs[0].data(), p.segs[1].data(), sizeof(uint4) * p.segs[0].size());
            printf("group %d %dx%d stride %d picture %d capacity %u bools %u/%u %s\n", g, W, H, stride, i, p.cap, p.n[0][0], p.n[1][0], ok ? "ok" : "MISMATCH");
            bad += !ok;
        }
    }
    printf("bad %d\n", bad);
    return bad;
}
