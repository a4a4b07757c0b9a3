/*
 * window_emu.h -- the body of the emulation programs of the window stages (mvrefs/mvrefs_emu.cpp, md_inter/md_inter_emu.cpp): a stage's
 * .hip itself (kernels and entry point, included by the program) on the CPU through the stand-in runtime of hip/hip_runtime.h, compared
 * with its host form: every byte of d_ext_out and d_cand with the guard bytes before and behind them, and the status words (the two buffers
 * are left out of the comparison for a grid the stage does not take: their contents are unspecified).  The grids are allocated to exactly
 * mi_rows x mi_stride records, the outputs as bytes.
 * argv[1]: a file holding int32 n_groups; per group int32 width, height, mi_stride, n_pics, offset, then per picture E::PAR parameter
 * bytes and the grids (svt_lf_mode_info, svt_mc_mode_info and, with E::EXT_GRID, svt_mi_inter_ext).  A group is one batch call; offset (0 or
 * 2) is the byte offset of d_ext_out and d_cand from a 16-byte boundary, in the device call and in the host call alike: 2 leaves the
 * records their own alignment only.
 * A program is a struct E: picture; PAR, EXT_GRID, STATUS_WORDS; desc(par, mi, mc, ext, ext_out, cand, status) -> picture, which leaves out
 * an output the parameter bytes do not ask for; device(ctx, n, pics, W, H, stride) and host(pic, W, H, stride), the two entry points.
 */
#pragma once
#include "emu_harness.h"
#define GUARD 64
/* `bytes` bytes at `offset` from a 16-byte boundary, GUARD + offset bytes of `fill` before them and GUARD behind */
struct guarded {
    uint8_t *base = nullptr;
    size_t   head = 0, bytes = 0;
    uint8_t  fill = 0;
    guarded() = default;
    guarded(const guarded &) = delete;
    void alloc(size_t n, int offset, uint8_t f) {
        head = GUARD + (size_t)offset; bytes = n; fill = f;
        if (posix_memalign((void **)&base, 16, head + bytes + GUARD)) abort();
        memset(base, fill, head + bytes + GUARD);
    }
    uint8_t *data() const { return base + head; }
    bool guards() const {
        bool ok = true;
        for (size_t k = 0; k < head; k++) ok = ok && base[k] == fill;
        for (size_t k = 0; k < GUARD; k++) ok = ok && base[head + bytes + k] == fill;
        return ok;
    }
    bool same(const guarded &o) const { return !memcmp(data(), o.data(), bytes); }
    ~guarded() { free(base); }
};
template <class E> struct pic_bufs {
    std::vector<svt_lf_mode_info> mi;
    std::vector<svt_mc_mode_info> mc;
    std::vector<svt_mi_inter_ext> ext;
    guarded               ext_out[2], cand[2]; /* [0]: the device's, [1]: the host form's */
    std::vector<uint32_t> status[2];
    uint8_t               par[E::PAR];
    typename E::picture desc(int k) {
        return E::desc(par, mi.data(), mc.data(), ext.data(), (svt_mi_inter_ext *)ext_out[k].data(), (svt_mvref_cand *)cand[k].data(), status[k].data());
    }
};
template <class E> int window_emu_main(int argc, char **argv) {
    static svt_hip_ctx ctx;
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    int32_t n_groups = 0;
    if (!f || fread(&n_groups, 4, 1, f) != 1) return 2;
    int bad = 0;
    for (int g = 0; g < n_groups; g++) {
        int32_t whn[5];
        if (fread(whn, 4, 5, f) != 5 || (whn[4] != 0 && whn[4] != 2)) return 3;
        const int    W = whn[0], H = whn[1], stride = whn[2], n_pics = whn[3], offset = whn[4];
        const size_t units = (size_t)stride * (H / 8);
        std::vector<pic_bufs<E>> P(n_pics);
        std::vector<typename E::picture> d(n_pics);
        for (int i = 0; i < n_pics; i++) {
            pic_bufs<E> &p = P[i];
            p.mi.resize(units); p.mc.resize(units); p.ext.resize(E::EXT_GRID ? units : 0);
            if (fread(p.par, 1, E::PAR, f) != E::PAR || fread(p.mi.data(), 8, units, f) != units || fread(p.mc.data(), 12, units, f) != units ||
                fread(p.ext.data(), 12, p.ext.size(), f) != p.ext.size())
                return 4;
            for (int k = 0; k < 2; k++) {
                p.ext_out[k].alloc(12 * units, offset, 0xA5); p.cand[k].alloc(32 * units, offset, 0x5A);
                p.status[k].assign(E::STATUS_WORDS + GUARD, 0x77777777u);
            }
            d[i] = p.desc(0);
        }
        const int r1 = E::device(&ctx, n_pics, d.data(), W, H, stride);
        for (int i = 0; i < n_pics; i++) {
            pic_bufs<E> &p = P[i];
            typename E::picture h = p.desc(1);
            const int  r2 = E::host(&h, W, H, stride);
            const bool taken = p.status[1][0] != SVT_MODES_BAD_GRID;
            bool       ok = !r1 && !r2 && p.status[0] == p.status[1];
            if (taken) ok = ok && p.ext_out[0].same(p.ext_out[1]) && p.cand[0].same(p.cand[1]);
            for (int k = 0; k < 2; k++) ok = ok && p.ext_out[k].guards() && p.cand[k].guards();
            printf("group %d %dx%d stride %d offset %d picture %d status", g, W, H, stride, offset, i);
            for (int k = 0; k < E::STATUS_WORDS; k++) printf(" %u/%u", p.status[0][k], p.status[1][k]);
            printf(" %s\n", ok ? "ok" : "MISMATCH");
            bad += !ok;
        }
    }
    printf("bad %d\n", bad);
    return bad;
}
