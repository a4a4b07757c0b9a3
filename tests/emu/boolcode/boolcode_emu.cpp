/*
 * boolcode_emu.cpp -- csrc/boolcode.hip itself (kernels and entry points, included below) on the CPU through the stand-in runtime of
 * tests/emu/hip/hip_runtime.h: random token / bool streams with and without segment lists (cuts behind EOB tokens, raw runs, empty segments)
 * through svt_hip_boolcode, compared byte for byte with svt_hip_boolcode_host.  argv[1]: a file holding one svt_bool_tables.
 * Streams reach past one tile of the chain kernel (8 192 bools) and past one tile of the carry kernel (256 words); the last two (tokens
 * and bools under a segment list, then raw bools alone) have more than 256 x 1024 items: a second pass of the tile scan with its carried sum.
 */
#include "boolcode.hip"
#include "emu_harness.h"
#include <random>
int main(int argc, char **argv) {
    static svt_hip_ctx ctx;
    svt_bool_tables tab;
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(&tab, sizeof tab, 1, f) != 1) return 2;
    svt_hip_boolcode_set_tables(&ctx, &tab);
    std::mt19937 rng(5);
    int bad = 0;
    for (int iter = 0; iter < 16; iter++) {
        const uint32_t nt = iter < 4 ? (uint32_t[]){0, 1, 700, 3000}[iter] : iter == 14 ? 150000 : iter == 15 ? 0 : rng() % 6000;
        const uint32_t nb = iter == 1 ? 0 : iter == 14 ? 130000 : iter == 15 ? 256 * 1024 + 777 : rng() % 9000;
        std::vector<uint32_t> tok(nt + 1); std::vector<uint16_t> bl(nb + 1);
        int c = 0;
        for (uint32_t i = 0; i < nt; i++) { /* plausible blocks: band from the position, EOB now and then */
            int t = rng() % 100 < 45 ? 0 : rng() % 100 < 40 ? 1 : 2 + rng() % 9;
            if (c > 0 && rng() % 9 == 0) t = 11;
            const int band = c == 0 ? 0 : c < 3 ? 1 : c < 6 ? 2 : c < 10 ? 3 : c < 21 ? 4 : 5, ctx6 = band ? rng() % 6 : rng() % 3;
            const uint32_t row = ((rng() % 16) * 6 + band) * 6 + ctx6;
            tok[i] = SVT_TOK_RECORD(t && t != 11 ? rng() & 0xffff : 0, row, t);
            c = t == 11 ? 0 : c + 1;
        }
        for (uint32_t i = 0; i < nb; i++) { const int p = 1 + rng() % 255; bl[i] = SVT_BOOL_RECORD((int)(rng() % 256) >= p, p); }
        std::vector<svt_bool_segment> segs;
        const bool use_segs = (iter >= 2 && (iter & 1)) || iter == 14;
        if (iter == 15) segs.push_back({0, nb, 1});
        else if (use_segs) { /* token runs cut behind EOB, bool runs, empty segments */
            uint32_t a = 0, bpos = 0;
            for (uint32_t i = 0; i < nt; i++) if (SVT_TOK_TOKEN(tok[i]) == 11 && rng() % 3 == 0) {
                segs.push_back({a, i + 1 - a, 0}); a = i + 1;
                if (rng() % 2 && bpos < nb) { const uint32_t n = rng() % 700 % (nb - bpos + 1); segs.push_back({bpos, n, 1}); bpos += n; }
                if (rng() % 5 == 0) segs.push_back({0, 0, (uint32_t)(rng() % 2)});
            }
            if (bpos < nb) segs.push_back({bpos, nb - bpos, 1});
        }
        const uint32_t cap = svt_hip_boolcode_capacity(nt * 22 + nb);
        std::vector<uint8_t> o1(cap + 8, 0xA5), o2(cap + 8, 0xA5);
        uint32_t s1 = 0, s2 = 0;
        const svt_bool_segment *sp = use_segs ? segs.data() : nullptr;
        int r1 = svt_hip_boolcode(&ctx, tok.data(), nt, bl.data(), nb, sp, (uint32_t)segs.size(), o1.data(), cap, &s1);
        int r2 = svt_hip_boolcode_host(&tab, tok.data(), nt, bl.data(), nb, sp, (uint32_t)segs.size(), o2.data(), cap, &s2);
        const bool ok = !r1 && !r2 && s1 == s2 && !memcmp(o1.data(), o2.data(), cap + 8);
        uint64_t items = use_segs ? 0 : nt;
        for (const svt_bool_segment &sg : segs) items += sg.count;
        printf("iter %d tokens %u bools %u segs %zu items %llu size %u/%u %s\n", iter, nt, nb, segs.size(), (unsigned long long)items, s1, s2, ok ? "ok" : "MISMATCH");
        bad += !ok;
    }
    printf("bad %d\n", bad);
    return bad;
}
