/* me_tables.h -- the sub-pel candidate tables, packed into immediates, and (emulation only) the reference's tables they are checked against. */
#ifndef SVT_ME_TABLES_H
#define SVT_ME_TABLES_H
#include "me_types.h"

enum { ME_PF = 0, ME_PB = 1, ME_PH = 2, ME_PJ = 3 }; /* where a candidate is read from: the integer region, or the half-pel plane B / H / J (me_subpel.h) */
/* The sub-pel candidate tables are packed into immediates so that no phase has to fetch them from memory:
 * a nibble holds plane (2 bits) | dx flag << 2 | dy flag << 3 (flag = -1 for the search tables, +1 for bi-pred). */
#define ME_HCAND_PACK 0x73BF2A15u
SVT_DEV void me_hcand_get(int cand, int *plane, int *dx, int *dy) {
    uint32_t n = (ME_HCAND_PACK >> (4 * cand)) & 15u;
    *plane = (int)(n & 3); *dx = -(int)((n >> 2) & 1); *dy = -(int)(n >> 3);
}
SVT_DEV uint32_t me_qtab_get(int method, int pos) { /* byte: first source nibble | second source nibble << 4 */
    const uint64_t v = method == 0 ? 0x25121AA5200A1005ull : method == 1 ? 0x5625A55E755F0554ull
                     : method == 2 ? 0xA51A9AAD0AA8BAAFull : 0x5EA5ADDE5FFDAFFEull;
    return (uint32_t)(v >> (8 * pos)) & 0xffu;
}
SVT_DEV uint32_t me_btab_get(int frac, int *has_b) {
    const uint64_t v = frac < 8 ? 0x6131212041011000ull : 0x9693928263033202ull;
    *has_b = (int)((0xFAFAu >> frac) & 1u);
    return (uint32_t)(v >> (8 * (frac & 7))) & 0xffu;
}
/* sign of the candidate displacement (L,R,T,B,TL,TR,BR,BL): half-pel moves by 2, quarter-pel by 1 quarter sample */
SVT_DEV void me_dmv_get(int i, int *sx, int *sy) {
    uint32_t n = (0x8A209164u >> (4 * i)) & 15u;
    *sx = (int)(n & 3) - 1; *sy = (int)(n >> 2) - 1;
}

#ifdef SVT_HOST_EMU /* data, not a path: the reference's tables; the kernel derives them arithmetically and the emulation checks that (me_tables_selfcheck, tests/emu/me_emu.c) */
/* raster index -> search (z-order) index, Codec/EbMotionEstimation.c:51-54 */
__attribute__((unused)) static
    const uint8_t me_tab32x32[16] = {0, 1, 4, 5, 2, 3, 6, 7, 8, 9, 12, 13, 10, 11, 14, 15};
__attribute__((unused)) static
    const uint8_t me_tab8x8[64] = {0,  1,  4,  5,  16, 17, 20, 21, 2,  3,  6,  7,  18, 19, 22, 23, 8,  9,  12, 13, 24, 25,
                                   28, 29, 10, 11, 14, 15, 26, 27, 30, 31, 32, 33, 36, 37, 48, 49, 52, 53, 34, 35, 38, 39,
                                   50, 51, 54, 55, 40, 41, 44, 45, 56, 57, 60, 61, 42, 43, 46, 47, 58, 59, 62, 63};

/* inverse maps: search (z-order) index -> raster index */
__attribute__((unused)) static
    const uint8_t me_inv32x32[16] = {0, 1, 4, 5, 2, 3, 6, 7, 8, 9, 12, 13, 10, 11, 14, 15};
__attribute__((unused)) static
    const uint8_t me_inv8x8[64] = {0,  1,  8,  9,  2,  3,  10, 11, 16, 17, 24, 25, 18, 19, 26, 27, 4,  5,  12, 13, 6,  7,
                                   14, 15, 20, 21, 28, 29, 22, 23, 30, 31, 32, 33, 40, 41, 34, 35, 42, 43, 48, 49, 56, 57,
                                   50, 51, 58, 59, 36, 37, 44, 45, 38, 39, 46, 47, 52, 53, 60, 61, 54, 55, 62, 63};
/* candidate tables ---------------------------------------------------------------------------------- */
/* half-pel candidates L,R,T,B,TL,TR,BR,BL relative to the integer position (pu_half_pel_refinement,
 * Codec/EbMotionEstimation.c:1076-1559), natural coordinates */
__attribute__((unused)) static
    const int8_t me_hcand[8][3] = {{ME_PB, -1, 0}, {ME_PB, 0, 0}, {ME_PH, 0, -1}, {ME_PH, 0, 0},
                                   {ME_PJ, -1, -1}, {ME_PJ, 0, -1}, {ME_PJ, 0, 0}, {ME_PJ, -1, 0}};
__attribute__((unused)) static
    const int8_t me_hdmv[8][2] = {{-2, 0}, {2, 0}, {0, -2}, {0, 2}, {-2, -2}, {2, -2}, {2, 2}, {-2, 2}};
/* quarter-pel pairs (set_quarter_pel_refinement_inputs_on_the_fly, :2290-2465), natural coordinates
 * relative to P = (mv + 2) >> 2; [method][position L,R,T,B,TL,TR,BR,BL][plane1,dx1,dy1,plane2,dx2,dy2] */
__attribute__((unused)) static
    const int8_t me_qtab[4][8][6] = {
        {{ME_PB, -1, 0, ME_PF, 0, 0}, {ME_PF, 0, 0, ME_PB, 0, 0}, {ME_PH, 0, -1, ME_PF, 0, 0}, {ME_PF, 0, 0, ME_PH, 0, 0},
         {ME_PB, -1, 0, ME_PH, 0, -1}, {ME_PH, 0, -1, ME_PB, 0, 0}, {ME_PH, 0, 0, ME_PB, 0, 0}, {ME_PB, -1, 0, ME_PH, 0, 0}},
        {{ME_PF, -1, 0, ME_PB, -1, 0}, {ME_PB, -1, 0, ME_PF, 0, 0}, {ME_PJ, -1, -1, ME_PB, -1, 0}, {ME_PB, -1, 0, ME_PJ, -1, 0},
         {ME_PH, -1, -1, ME_PB, -1, 0}, {ME_PB, -1, 0, ME_PH, 0, -1}, {ME_PB, -1, 0, ME_PH, 0, 0}, {ME_PH, -1, 0, ME_PB, -1, 0}},
        {{ME_PJ, -1, -1, ME_PH, 0, -1}, {ME_PH, 0, -1, ME_PJ, 0, -1}, {ME_PF, 0, -1, ME_PH, 0, -1}, {ME_PH, 0, -1, ME_PF, 0, 0},
         {ME_PB, -1, -1, ME_PH, 0, -1}, {ME_PH, 0, -1, ME_PB, 0, -1}, {ME_PH, 0, -1, ME_PB, 0, 0}, {ME_PB, -1, 0, ME_PH, 0, -1}},
        {{ME_PH, -1, -1, ME_PJ, -1, -1}, {ME_PJ, -1, -1, ME_PH, 0, -1}, {ME_PB, -1, -1, ME_PJ, -1, -1}, {ME_PJ, -1, -1, ME_PB, -1, 0},
         {ME_PH, -1, -1, ME_PB, -1, -1}, {ME_PB, -1, -1, ME_PH, 0, -1}, {ME_PB, -1, 0, ME_PH, 0, -1}, {ME_PH, -1, -1, ME_PB, -1, 0}}};
__attribute__((unused)) static
    const int8_t me_qdmv[8][2] = {{-1, 0}, {1, 0}, {0, -1}, {0, 1}, {-1, -1}, {1, -1}, {1, 1}, {-1, 1}};
/* bi-pred quarter-pel compensation pairs (quarter_pel_compensation, :3358-3453), by frac_pos */
__attribute__((unused)) static
    const int8_t me_btab[16][6] = {
        {ME_PF, 0, 0, -1, 0, 0}, {ME_PF, 0, 0, ME_PB, 0, 0}, {ME_PB, 0, 0, -1, 0, 0}, {ME_PB, 0, 0, ME_PF, 1, 0},
        {ME_PF, 0, 0, ME_PH, 0, 0}, {ME_PB, 0, 0, ME_PH, 0, 0}, {ME_PB, 0, 0, ME_PJ, 0, 0}, {ME_PB, 0, 0, ME_PH, 1, 0},
        {ME_PH, 0, 0, -1, 0, 0}, {ME_PH, 0, 0, ME_PJ, 0, 0}, {ME_PJ, 0, 0, -1, 0, 0}, {ME_PJ, 0, 0, ME_PH, 1, 0},
        {ME_PH, 0, 0, ME_PF, 0, 1}, {ME_PH, 0, 0, ME_PB, 0, 1}, {ME_PJ, 0, 0, ME_PB, 0, 1}, {ME_PH, 1, 0, ME_PB, 0, 1}};

/* returns 0 when every packed / arithmetic table decodes to the reference tables above */
static inline int me_tables_selfcheck(void) {
    for (int i = 0; i < 64; i++) if (me_z8(i) != me_tab8x8[i] || me_inv8x8[me_z8(i)] != i) return 1;
    for (int i = 0; i < 16; i++) if (me_z4(i) != me_tab32x32[i] || me_inv32x32[me_z4(i)] != i) return 2;
    for (int i = 0; i < 8; i++) {
        int pl, dx, dy, sx, sy;
        me_hcand_get(i, &pl, &dx, &dy);
        if (pl != me_hcand[i][0] || dx != me_hcand[i][1] || dy != me_hcand[i][2]) return 3;
        me_dmv_get(i, &sx, &sy);
        if (2 * sx != me_hdmv[i][0] || 2 * sy != me_hdmv[i][1] || sx != me_qdmv[i][0] || sy != me_qdmv[i][1]) return 4;
    }
    for (int m = 0; m < 4; m++)
        for (int i = 0; i < 8; i++) {
            uint32_t       v = me_qtab_get(m, i);
            const int8_t *e = me_qtab[m][i];
            if ((int)(v & 3) != e[0] || -(int)((v >> 2) & 1) != e[1] || -(int)((v >> 3) & 1) != e[2]) return 5;
            if ((int)((v >> 4) & 3) != e[3] || -(int)((v >> 6) & 1) != e[4] || -(int)((v >> 7) & 1) != e[5]) return 6;
        }
    for (int f = 0; f < 16; f++) {
        int            hb;
        uint32_t       v = me_btab_get(f, &hb);
        const int8_t *e = me_btab[f];
        if ((int)(v & 3) != e[0] || (int)((v >> 2) & 1) != e[1] || (int)((v >> 3) & 1) != e[2]) return 7;
        if (hb != (e[3] >= 0)) return 8;
        if (hb && ((int)((v >> 4) & 3) != e[3] || (int)((v >> 6) & 1) != e[4] || (int)((v >> 7) & 1) != e[5])) return 9;
    }
    return 0;
}
#endif
#endif
