/*
 * modeinfo_emu.cpp -- csrc/modeinfo.hip itself (kernels and entry points, included below) on the CPU through the stand-in runtime of
 * tests/emu/hip/hip_runtime.h, compared with svt_hip_modes_kf_picture: bool records up to the capacity, the guard words behind them, every
 * segment record, the bool total.  argv[1]: a file holding one svt_modes_tables, then int32 n_groups; per group int32 width, height,
 * n_pics, then per picture int32 capacity, the grid (mi_rows x mi_cols records), the eob map (uint16), the tokeniser's offsets (uint32).
 * A group is one batch call.
 */
#include "modeinfo.hip"
#include "emu_harness.h"
struct pic_bufs {
    std::vector<svt_lf_mode_info> mi;
    std::vector<uint16_t> emap, bools[2];
    std::vector<uint32_t> tok_off, n[2];
    std::vector<uint4> segs[2]; /* (16-byte aligned by the allocator's alignment of uint4) */
    uint32_t cap;
};
int main(int argc, char **argv) {
    static svt_hip_ctx ctx;
    svt_modes_tables tab;
    FILE *f = fopen(argv[1], "rb");
    int32_t n_groups = 0;
    if (!f || fread(&tab, sizeof tab, 1, f) != 1 || fread(&n_groups, 4, 1, f) != 1) return 2;
    svt_hip_modes_set_tables(&ctx, &tab);
    int bad = 0;
    for (int g = 0; g < n_groups; g++) {
        int32_t whn[3];
        if (fread(whn, 4, 3, f) != 3) return 3;
        const int W = whn[0], H = whn[1], n_pics = whn[2], units = (W / 8) * (H / 8), map_n = (W / 4) * (H / 4) * 3 / 2;
        const uint32_t n_seg = svt_hip_modes_segments(W, H);
        std::vector<pic_bufs> P(n_pics);
        std::vector<svt_modes_picture> d(n_pics);
        for (int i = 0; i < n_pics; i++) {
            int32_t cap;
            pic_bufs &p = P[i];
            p.mi.resize(units); p.emap.resize(map_n); p.tok_off.resize(map_n);
            if (fread(&cap, 4, 1, f) != 1 || fread(p.mi.data(), 8, units, f) != (size_t)units || fread(p.emap.data(), 2, map_n, f) != (size_t)map_n ||
                fread(p.tok_off.data(), 4, map_n, f) != (size_t)map_n)
                return 4;
            p.cap = (uint32_t)cap;
            for (int k = 0; k < 2; k++) {
                p.bools[k].assign(p.cap + 64, 0xA5A5); p.n[k].assign(4, 0x77777777u);
                p.segs[k].assign(n_seg * 3 / 4 + 8, make_uint4(0x5A5A5A5Au, 0x5A5A5A5Au, 0x5A5A5A5Au, 0x5A5A5A5Au));
            }
            d[i] = {p.mi.data(), p.emap.data(), p.tok_off.data(), p.bools[0].data(), (svt_bool_segment *)p.segs[0].data(), p.n[0].data(), p.cap, 0};
        }
        const int r1 = svt_hip_modes_kf_batch_device(&ctx, n_pics, d.data(), W, H, W / 8);
        for (int i = 0; i < n_pics; i++) {
            pic_bufs &p = P[i];
            svt_modes_picture h = {p.mi.data(), p.emap.data(), p.tok_off.data(), p.bools[1].data(), (svt_bool_segment *)p.segs[1].data(), p.n[1].data(), p.cap, 0};
            const int  r2 = svt_hip_modes_kf_picture(&tab, &h, W, H, W / 8);
            const bool ok = !r1 && !r2 && p.n[0] == p.n[1] && p.bools[0] == p.bools[1] && !memcmp(p.segs[0].data(), p.segs[1].data(), sizeof(uint4) * p.segs[0].size());
            printf("group %d %dx%d picture %d capacity %u bools %u/%u %s\n", g, W, H, i, p.cap, p.n[0][0], p.n[1][0], ok ? "ok" : "MISMATCH");
            bad += !ok;
        }
    }
    printf("bad %d\n", bad);
    return bad;
}
